// dt_cut.hpp -- the host cut planner (dt_cut.cpp): where a long document's replay may be cut into
// LV segments.  Plain host C++: no HIP type appears here.
#pragma once
#include <array>
#include <cstdint>
#include <utility>
#include <vector>

#include "dt_host.hpp"

namespace dtgpu {

// ---- cut replay (dt_replay.hip "segments") ------------------------------------------------------
// A long document replays as segments on several waves, cut at LVs v where the prefix [0, v)
// is one version ({v-1}) and every later entry has it in its history: the reference fast-forwards
// exactly there (merge.rs:811-840) because the text at v is then a plain string.  Cuts go at op
// run starts (every command boundary is one), spread so that the segments hold about equal op
// runs.  A segment's placeholders bound the text at its start: inserts - deletes + the deletes
// that are concurrent with some other op (a delete can hit an already deleted item only then).
struct SegCut { uint32_t lo, hi, u; uint64_t ins; };   // LV range, placeholders, inserted chars in range
struct SegInput {
    uint64_t n_lv = 0;
    std::vector<std::pair<uint64_t, uint64_t>> ent;   // entries [start, end) in LV order
    std::vector<uint32_t> poff;                       // parents CSR (ent.size() + 1)
    std::vector<uint64_t> par;
    std::vector<std::array<uint64_t, 3>> ops;         // op runs (lv, len, kind: 0 ins, 1 del) in LV order
};
struct SegSettings { bool on; uint64_t ops_per_seg; uint32_t max_seg, w_op; };

std::vector<std::pair<uint64_t, uint64_t>> cut_ranges(const SegInput &in);
std::vector<SegCut> plan_segments(const SegInput &in, const SegSettings &cfg);
// Cut replay inputs from a host oplog (one long document).
void seg_input_from_log(const HostOpLog &o, SegInput &si);

}  // namespace dtgpu
