// dt_merge.hpp -- batched iter_xf_operations_from / ListBranch::merge over resident documents
// (dtgpu_decode_xf_from, dtgpu_merge.cpp): what the projection keeps for a merge request, the
// staging form of a merge batch, and the two small kernels that translate LVs between a base
// document and a request's projection (dt_merge.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/dtgpu.h"
#include "dt_decoded.hpp"
#include "dt_devbuf.hpp"
#include "dt_device.hpp"
#include "dt_history.hpp"

struct dtgpu_batch;

namespace dtgpu {

// A projection made for merge requests keeps its mark words (reach / nb per base entry: the
// monotone LV map, dt_mark.hpp map_lv) and its descriptors on the device.
struct HistKeep {
    DevBuf<uint32_t> scr;
    DevBuf<HistDesc> hd;
};
// dtgpu_decode_history with `keep`: the outputs keep the base document's graph entries
// (HistParams::keep_entries) and the mark words stay alive in *keep.
dtgpu_status decode_history(const dtgpu_decoded *B, const uint32_t *doc, const uint64_t *versions,
                            const size_t *version_off, size_t n, float *ms, dtgpu_decoded **out, HistKeep *keep);

// The merge form of a device-staged batch: document i of the handle is the projection of request
// i; from[from_off[i] .. from_off[i + 1]) is its `from` in projected LVs (device words); skip[i]
// != 0 leaves the request out of the pass.
// The most LVs a request's `from` may hold once sorted and without repeats: plan_kernel_xf reduces
// the set to a frontier on one wave, serially (a frontier itself has at most 64 LVs, one per chain);
// a longer set is DTGPU_DECODE_DEFER.
constexpr uint32_t MERGE_MAX_FROM = 256;

struct XfStage {
    const uint32_t *d_from = nullptr;
    std::vector<uint64_t> from_off;
    std::vector<uint8_t> skip;
    std::vector<uint32_t> xf_first, n_xf;   // out: per request, the first reported command, the reported LVs
};
// One pass of a merge batch on its stream, timed: prep, plan, replay milliseconds.
dtgpu_status run_xf_pass(dtgpu_batch *B, float ms[3]);

struct MergeParams {
    // the base documents and the requests' mark words
    const uint32_t *b_ent;
    const uint32_t *scr;
    const HistDesc *hd;
    uint32_t n;
    // base -> projected: the requests' `from`
    const uint32_t *from;       // base LVs
    uint32_t *from_out;         // projected LVs
    const uint64_t *from_off;   // n + 1
    const uint32_t *ok;         // per request: 1 = translate
    // projected -> base: the reported records
    const Cmd *cmds;
    const uint32_t *xf;         // transformed position per projected LV
    const uint64_t *cmd_off, *lv_off, *rec_off;   // per request
    const uint32_t *ncmd, *first, *n_rec;
    uint32_t *rec;              // {base lv, pos} pairs
};
int launch_merge_from(const MergeParams &p, void *stream);
int launch_merge_records(const MergeParams &p, void *stream);

}  // namespace dtgpu
