// dt_summary.hpp -- host/device layout of the batched version-summary intersection
// (dt_summary.hip): CausalGraph::intersect_with_summary (src/causalgraph/summary.rs:175-264) for a
// batch of (resident document, peer summary) requests, one 64-lane wavefront per request.
//
// A peer names versions as (agent name, seq ranges).  A request's entries are resolved to agent ids
// of its document, every range is clipped against that agent's runs, and each known piece gives one
// LV (its last seq's, summary.rs:242).  Those LVs and the caller's extra LVs are the request's LV
// set in HistParams::req, which the history mark sweep (dt_mark.hpp) reduces to its dominators
// exactly as it reduces a caller's request: find_dominators is not restated here.  The uncovered
// stretches of every range are the remainder, (entry, start, end) records in visiting order.
//
// Two launches, as the history projection has: sum_count_kernel resolves the names and counts each
// request's known pieces; the host prefix-sums the counts into the LV-set and remainder arenas;
// sum_emit_kernel writes both.  Only the per-request counts visit the host.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "dt_history.hpp"

namespace dtgpu {

struct SumDesc {
    uint64_t ent0, rng0;          // first entry / first range of the request (indexes into the flattened arrays)
    uint32_t n_ent, n_rng;
    uint64_t ext_off;             // extra LVs in SumParams::ext
    uint32_t n_ext, skip;         // skip: the status to report without intersecting (0: intersect)
    uint64_t eag_off;             // n_ent words of SumParams::eag: entry -> agent id (NONE: unknown name)
    uint64_t pc_off;              // 2 * c_known pairs of SumParams::pieces (the pieces, and where a re-ordered range is ranked into)
    uint64_t rem_off;             // c_rem triples of SumParams::rem
    uint32_t c_known, c_rem;      // emit launch: the reservations
};

struct SumCounts {
    uint32_t status;
    uint32_t n_known;             // count launch: known pieces; emit launch: the same, recounted
    uint32_t n_rem;               // emit launch: remainder records
    uint32_t n_resorted;          // emit launch: ranges whose pieces were not in seq order
};

struct SumParams {
    HistParams H;                 // the base arenas; H.docs per request (req_off, n_req: the LV set to write); H.req is written
    const SumDesc *docs;
    const uint8_t *names;         // all entries' name bytes
    const uint64_t *name_off;     // entries + 1
    const uint64_t *range_off;    // entries + 1, in ranges
    const uint64_t *ranges;       // pairs {start, end}
    const uint32_t *range_ent;    // per range: its entry's index within its request
    const uint32_t *ext;          // extra LVs (clamped to 32 bits: anything past the document fails the mark's check)
    uint32_t *eag;
    uint64_t *pieces;
    uint64_t *rem;
    uint32_t *req;                // = H.req, writable
    SumCounts *counts;
    uint32_t n_docs, pad;
};

int launch_sum_count(const SumParams &p, void *stream);
int launch_sum_emit(const SumParams &p, void *stream);

// AgentAssignment::summarize_versions (summary.rs:119-132) over agent runs in any order: per agent
// id, its seq ranges sorted and merged where adjacent (merge_spans).  run(i) = {agent, seq, len}.
template <typename F>
inline std::vector<std::vector<std::pair<uint64_t, uint64_t>>> summarize_runs(size_t n_agents, size_t n_runs, F run) {
    std::vector<std::vector<std::pair<uint64_t, uint64_t>>> by(n_agents);
    for (size_t i = 0; i < n_runs; i++) {
        uint32_t a;
        uint64_t seq, len;
        run(i, a, seq, len);
        if (a < n_agents && len) by[a].emplace_back(seq, seq + len);
    }
    for (auto &v : by) {
        std::sort(v.begin(), v.end());
        size_t k = 0;
        for (size_t i = 0; i < v.size(); i++) {
            if (k && v[k - 1].second == v[i].first) v[k - 1].second = v[i].second;
            else v[k++] = v[i];
        }
        v.resize(k);
    }
    return by;
}


// One summary into the caller's buffers (dtgpu_oplog_summarize's protocol): agents without ranges are
// omitted.  name(a, ptr, len) gives agent a's name.  Returns false when a buffer is too small.
template <typename F>
inline bool write_summary(const std::vector<std::vector<std::pair<uint64_t, uint64_t>>> &by, F name, uint8_t *names,
                          size_t names_cap, size_t *name_off, size_t *range_off, size_t entry_cap, uint64_t *ranges,
                          size_t range_cap, size_t sizes[3]) {
    size_t ne = 0, nb = 0, nr = 0;
    bool fit = true;
    for (size_t a = 0; a < by.size(); a++) {
        if (by[a].empty()) continue;
        const uint8_t *p = nullptr;
        size_t len = 0;
        name(a, p, len);
        if (name_off) { if (ne < entry_cap) name_off[ne] = nb; else fit = false; }
        if (range_off) { if (ne < entry_cap) range_off[ne] = nr; else fit = false; }
        if (names) { if (nb + len <= names_cap) std::copy(p, p + len, names + nb); else fit = false; }
        for (const auto &r : by[a]) {
            if (ranges) { if (nr < range_cap) { ranges[2 * nr] = r.first; ranges[2 * nr + 1] = r.second; } else fit = false; }
            nr++;
        }
        nb += len;
        ne++;
    }
    if (name_off && ne <= entry_cap) name_off[ne] = nb;
    if (range_off && ne <= entry_cap) range_off[ne] = nr;
    if (sizes) { sizes[0] = ne; sizes[1] = nb; sizes[2] = nr; }
    return fit;
}

}  // namespace dtgpu
