// dt_decoded.hpp -- the decoder handle (dtgpu_decoded): device arenas of a decoded batch (and the
// two helpers every producer of such arenas uses: the 256-B alignment and the CRC combine table),
// shared by the decode API (dtgpu_decode.cpp) and the device-staged checkout batches
// (dtgpu_stage.cpp), which read the decoded oplogs in place.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "dt_decode.hpp"
#include "dt_devbuf.hpp"
#include "dt_request_shape.hpp"

using dtgpu::DecodeDesc;
using dtgpu::DecodeParams;
using dtgpu::DecodeResult;
using dtgpu::DevBuf;

namespace dtgpu {

// Arena offsets of documents and patches are 256-B aligned.
inline uint64_t align256(uint64_t x) { return (x + 255) & ~uint64_t(255); }

inline uint32_t multmodp_host(uint32_t a, uint32_t b) {
    if (!a) return 0;
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1u) ? (b >> 1) ^ 0x82F63B78u : b >> 1;
    }
    return p;
}

// x^(2^k) mod the CRC-32C polynomial, k < 32: the table the kernels' CRC segment combine reads
inline void crc_x2n(uint32_t (&x2n)[32]) {
    x2n[0] = 1u << 30;
    for (int k = 1; k < 32; k++) x2n[k] = multmodp_host(x2n[k - 1], x2n[k - 1]);
}

}  // namespace dtgpu

struct dtgpu_decoded {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    size_t n = 0;
    uint64_t in_bytes = 0;
    float last_ms = 0;
    std::vector<DecodeDesc> desc;
    std::vector<DecodeResult> res;
    DevBuf<uint8_t> in, lz, content;
    DevBuf<uint32_t> aruns, alist, pre, ops, ent, poff, par, cbyte, agents, ver;
    DevBuf<uint32_t> lz_big, lz_pre;   // documents whose LZ4 block lz4_kernel decompresses, its verdicts
    DevBuf<uint32_t> fill, fill_n, fill_doc;   // deferred per-LV offsets (DecodeParams::fill)
    DevBuf<uint32_t> order;                    // decode_kernel's dispatch order (DecodeParams::order)
    // dtgpu_decode_add results: the merged oplogs (not re-decodable); each merge's status and the
    // patch's version are in `fronts`, read from ffr within the call
    bool merged = false;
    DevBuf<uint32_t> ffr;
    // dtgpu_decode_run has run (a decoded handle's arrays exist); dtgpu_decode_history results (hfr
    // allocated): each output's status and its request reduced to a frontier, in its base
    // document's LVs, are in `fronts`, read from hfr within the call
    bool ran = false;
    DevBuf<uint32_t> hfr;
    dtgpu::FrontierSet fronts;
    DevBuf<DecodeDesc> d_desc;
    DevBuf<DecodeResult> d_res;
    DecodeParams P{};
    ~dtgpu_decoded() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
    }
};
