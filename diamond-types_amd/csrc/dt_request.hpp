// dt_request.hpp -- the host scaffold of the per-request calls over a resident dtgpu_decoded:
// dtgpu_decode_add and dtgpu_decode_history (dtgpu_decode.cpp), dtgpu_decode_encode_from
// (dtgpu_patch.cpp), dtgpu_decode_intersect / dtgpu_decode_encode_from_summaries
// (dtgpu_summary.cpp) and dtgpu_decode_xf_from (dtgpu_merge.cpp).
//
// A call supplies its kernels, their descriptors and its arena layout.  It gets from here: the
// request's shape check and LV packing and the FrontierSet its *_result function reads
// (dt_request_shape.hpp, no HIP runtime needed), the frontiers' copy to the host
// (fetch_frontiers), a stream and timing events that clean up after themselves, the base document's
// half of the mark launch's descriptors (mark_setup, hist_params_base), and DTGPU_CK (dt_devbuf.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/dtgpu.h"
#include "dt_decoded.hpp"
#include "dt_history.hpp"
#include "dt_request_shape.hpp"

namespace dtgpu {

// A non-blocking stream of the call's own.
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
};

// N events: record(i, s) on a stream, ms(i, j) between two recorded ones once the stream is synchronised.
template <int N>
struct Events {
    hipEvent_t e[N] = {};
    Events() = default;
    Events(const Events &) = delete;
    Events &operator=(const Events &) = delete;
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    hipError_t create(unsigned flags = hipEventDefault) {
        for (hipEvent_t &x : e)
            if (hipError_t err = hipEventCreateWithFlags(&x, flags)) return err;
        return hipSuccess;
    }
    hipError_t record(int i, hipStream_t s) { return hipEventRecord(e[i], s); }
    hipError_t ms(int i, int j, float *out) { return hipEventElapsedTime(out, e[i], e[j]); }
};

// (B, doc, LV-set CSR) is a request batch a per-request call can stage (request_ok over a handle).
inline bool request_ok(const dtgpu_decoded *B, const uint32_t *doc, const uint64_t *lv, const size_t *off, size_t n) {
    return B && request_ok(B->merged || B->ran, B->n, doc, lv, off, n);
}

// The frontiers a kernel left in d_front (DECODE_MAX_FRONTIER words per request) into fs.front: one
// blocking copy after the call's last synchronisation, timed apart under DTGPU_STAGE_PROF.  The
// caller then fills fs.status / fs.n_front by its own rule.
inline hipError_t fetch_frontiers(FrontierSet &fs, const uint32_t *d_front, size_t n) {
    fs.assign(n);
    stage_prof(nullptr);
    const hipError_t e = n ? hipMemcpy(fs.front.get(), d_front, size_t(DECODE_MAX_FRONTIER) * n * 4, hipMemcpyDeviceToHost) : hipSuccess;
    stage_prof("frontiers to host");
    return e;
}

// The mark launch's per-request descriptors: the base document's arenas and counts, where the mark
// words live (LDS or HBM scratch, by the history projection's rule and its
// DTGPU_HISTORY_LDS_ENTRIES override), the scratch and frontier slots.  req_off / n_req are the
// caller's to fill (pack_sets, or a kernel's counts).  This and hist_params_base are the only
// place that fills the b_* half of a HistDesc / HistParams.
struct MarkSetup {
    std::vector<HistDesc> hd;
    uint64_t scr_words = 0;     // HistParams::scr
    uint32_t lds_entries = 0;   // dynamic LDS of the mark launch, in words
};
void mark_setup(const dtgpu_decoded &B, const uint32_t *doc, size_t n, MarkSetup &ms);
// The base arenas of B in H.
void hist_params_base(const dtgpu_decoded &B, HistParams &H);

// dtgpu_decode_encode_from from its mark launch on (dtgpu_patch.cpp): the requests' LV sets are
// d_req and their descriptors d_hd (= ms.hd with req_off / n_req filled), both already in HBM and
// ready on stream s.  mark (may be null): the patches' FrontierSet with the mark launch's status
// (before the encoder's own) in place of the patch's.
dtgpu_status patches_from_requests(const dtgpu_decoded *B, const uint32_t *doc, size_t n, uint32_t flags,
                                   const MarkSetup &ms, const HistDesc *d_hd, const uint32_t *d_req, hipStream_t s,
                                   float *ms_out, dtgpu_patches **out, FrontierSet *mark = nullptr);

}  // namespace dtgpu
