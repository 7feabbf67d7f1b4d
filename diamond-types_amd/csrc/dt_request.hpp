// dt_request.hpp -- host staging shared by the entry points that run the history mark sweep over a
// batch of (resident document, LV set) requests: dtgpu_decode_encode_from (dtgpu_decode.cpp), whose
// LV sets come from the caller, and the summary entry points (dtgpu_summary.cpp), whose LV sets
// dt_summary.hip writes in HBM.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/dtgpu.h"
#include "dt_decoded.hpp"
#include "dt_history.hpp"

namespace dtgpu {

// The mark launch's per-request descriptors: the base document's arenas and counts, where the mark
// words live (LDS or HBM scratch, by the history projection's rule and its
// DTGPU_HISTORY_LDS_ENTRIES override), the scratch and frontier slots.  req_off / n_req are the
// caller's to fill.
struct MarkSetup {
    std::vector<HistDesc> hd;
    uint64_t scr_words = 0;     // HistParams::scr
    uint32_t lds_entries = 0;   // dynamic LDS of the mark launch, in words
};
void mark_setup(const dtgpu_decoded &B, const uint32_t *doc, size_t n, MarkSetup &ms);
// The base arenas of B in H.
void hist_params_base(const dtgpu_decoded &B, HistParams &H);

// dtgpu_decode_encode_from from its mark launch on: the requests' LV sets are d_req and their
// descriptors d_hd (= ms.hd with req_off / n_req filled), both already in HBM and ready on stream s.
// mark (may be null): what the mark launch left per request, on the host -- its status (before the
// encoder's own), the reduced frontier's width and LVs (DECODE_MAX_FRONTIER slots each).
struct MarkOut { std::vector<uint32_t> status, n_front, front; };
dtgpu_status patches_from_requests(const dtgpu_decoded *B, const uint32_t *doc, size_t n, uint32_t flags,
                                   const MarkSetup &ms, const HistDesc *d_hd, const uint32_t *d_req, hipStream_t s,
                                   float *ms_out, dtgpu_patches **out, MarkOut *mark = nullptr);

}  // namespace dtgpu
