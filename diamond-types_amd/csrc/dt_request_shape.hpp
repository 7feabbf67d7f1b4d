// dt_request_shape.hpp -- the part of the request scaffold (dt_request.hpp) that needs no HIP
// runtime: the shape check of a batch of (resident document, LV set) requests, the packing of the
// LV sets into the u32 words the kernels read, and the per-request result triple {status, reduced
// frontier width, reduced frontier} with its one reader.  tests/sanitize/request_shapes.cpp builds
// this header alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "../../include/dtgpu.h"
#include "dt_decode.hpp"

namespace dtgpu {

// An LV as the kernels hold it (an LV past 32 bits names no op of a resident document: it clamps to
// the word every kernel rejects as out of range).
inline uint32_t lv32(uint64_t lv) { return uint32_t(std::min<uint64_t>(lv, 0xFFFFFFFFull)); }

// n LV sets as a CSR -- set i is lv[off[i] .. off[i + 1]); off[0] need not be 0 -- are well formed:
// the offsets ascend and lv is there when any set has an LV.
inline bool sets_ok(const uint64_t *lv, const size_t *off, size_t n) {
    if (!n) return true;
    if (!off) return false;
    for (size_t i = 0; i < n; i++)
        if (off[i + 1] < off[i]) return false;
    return off[n] == off[0] || lv;
}

// doc[0 .. n) name documents of a base handle of base_n documents whose arrays exist (base_ready:
// a decoded handle that has run, or a merged one).
inline bool docs_ok(bool base_ready, size_t base_n, const uint32_t *doc, size_t n) {
    if (!base_ready || (n && !doc)) return false;
    for (size_t i = 0; i < n; i++)
        if (doc[i] >= base_n) return false;
    return true;
}

// The (document, LV set) request batch of every per-request call.
inline bool request_ok(bool base_ready, size_t base_n, const uint32_t *doc, const uint64_t *lv, const size_t *off, size_t n) {
    return docs_ok(base_ready, base_n, doc, n) && sets_ok(lv, off, n);
}

// The sets as the kernels read them: every LV clamped (lv32) into req, which starts at the first
// set whatever off[0] is; set i is req[d[i].*req_off .. + d[i].*n_req).
template <class D>
void pack_sets(const uint64_t *lv, const size_t *off, size_t n, std::vector<uint32_t> &req, D *d, uint64_t D::*req_off,
               uint32_t D::*n_req) {
    req.resize(n ? off[n] - off[0] : 0);
    for (size_t i = 0; i < n; i++) {
        d[i].*req_off = off[i] - off[0];
        d[i].*n_req = uint32_t(off[i + 1] - off[i]);
    }
    for (size_t k = 0; k < req.size(); k++) req[k] = lv32(lv[off[0] + k]);
}

// What a per-request call leaves on the host for each request: its status and its LV set reduced to
// a frontier (base LVs, ascending; DECODE_MAX_FRONTIER words per request, as the kernels write
// them).  The producer zeroes n_front[i] wherever it has no frontier to give.
struct FrontierSet {
    std::vector<uint32_t> status, n_front;
    std::unique_ptr<uint32_t[]> front;   // (not zeroed: a copy from the device fills it)
    void assign(size_t n) {
        status.assign(n, 0);
        n_front.assign(n, 0);
        front.reset(new uint32_t[size_t(DECODE_MAX_FRONTIER) * n]);
    }
    // Request i: *n_frontier (may be null) is the frontier's width, frontier[0 .. min(cap, width))
    // its LVs; returns the request's status.  A bad index, or a null buffer with a cap:
    // DTGPU_ERR_ARG, and *n_frontier is left alone.
    dtgpu_status read(size_t i, uint64_t *frontier, size_t cap, size_t *n_frontier) const {
        if (i >= status.size() || (!frontier && cap)) return DTGPU_ERR_ARG;
        const size_t k = n_front[i];
        if (n_frontier) *n_frontier = k;
        for (size_t j = 0; j < k && j < cap; j++) frontier[j] = front[size_t(DECODE_MAX_FRONTIER) * i + j];
        return dtgpu_status(status[i]);
    }
};

}  // namespace dtgpu
