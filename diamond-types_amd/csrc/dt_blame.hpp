// dt_blame.hpp -- host/device layout of the batched blame (dt_blame.hip): who wrote each character.
//
// The blame of a document at the version it checks out is the sequence of maximal runs (lv, len,
// agent, seq) in text order: character k of a run was inserted by LV lv + k = (agent, seq + k).
// The replay already knows it for a moment -- a segment's visible items in document order are a
// list of LVs (materialise_src, dt_replay.hip), the fast-forward path's final piece list is LV
// ranges (dt_ff.hpp) -- so a blame batch keeps that list and turns it into runs:
//
//   tracker documents  every uncut document is staged as a segment group of one (seg_lo = 0,
//                      seg_hi = ~0, seg_u = 0, src_off / src_cap set), so its replay writes the
//                      source list and the combine step the text; a cut document's final list is
//                      its last segment's, resolved in place by the combine step
//   linear documents   the final piece list of dt_ff.hip, split at agent-run boundaries
//
// Kernels of one pass: blame_len_kernel before the combine step (it overwrites a group of one's
// list length with the text's byte length), then blame_bits_kernel (a bitmap of the LVs at which
// (agent, seq) does not continue the LV before: one load per character instead of a binary
// search) and blame_runs_kernel in counting mode.  The run arena is sized from the counts, and
// blame_runs_kernel in emit mode writes one 16-byte run per head; only the runs are read back.
#pragma once
#include <stdint.h>

#include "dt_device.hpp"
#include "dt_ff.hpp"

namespace dtgpu {

constexpr uint32_t BLAME_NONE = 0;      // a failed document: no runs
constexpr uint32_t BLAME_TRACKER = 1;   // the final source list of the replay
constexpr uint32_t BLAME_FF = 2;        // the final piece list of the fast-forward path

struct BlameRun { uint32_t lv, len, agent, seq; };   // = dtgpu_blame_run (include/dtgpu.h)

struct BlameDoc {          // per document of the batch
    uint64_t src_off;      // tracker: the final list, into src (uint32 units)
    uint64_t arun_off;     // into aruns (uint32 units): quads lv_start, name rank, seq_start, agent
    uint64_t bits_off;     // into bits (words): one bit per LV
    uint32_t n_aruns, n_lv;
    uint32_t kind;         // BLAME_*
    uint32_t last;         // tracker: docs[] / results[] index of the last segment; ff: FFDoc index
    uint32_t cap;          // tracker: the final list's capacity in entries
    uint32_t pad;
};

struct BlameParams {
    const BlameDoc *docs;
    uint32_t n_docs;
    const uint32_t *aruns;
    const uint32_t *src;
    const DocResult *results;   // results[i]: the document's status after the pass
    uint32_t *bits;
    uint32_t *len;              // per document: entries of its final list (tracker)
    uint32_t *count;            // per document: runs; [n_docs + i]: characters
    const uint64_t *run_off;    // emit mode: per document, its first run's slot
    BlameRun *runs;
    // the fast-forward path's final lists (dt_ff.hpp)
    const FFDoc *ff_docs;
    const uint32_t *pa, *pb, *ca, *cb;
};

// Before the combine step: every tracker document's final list length.
int launch_blame_len(const BlameParams &p, void *stream);
// After the pass: the boundary bitmaps, then the runs counted (p.count).
int launch_blame_count(const BlameParams &p, void *stream);
// The runs written (p.run_off, p.runs sized from the counts).
int launch_blame_emit(const BlameParams &p, void *stream);

}  // namespace dtgpu
