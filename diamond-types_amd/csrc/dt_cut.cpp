// dt_cut.cpp -- the host cut planner: cut ranges of a decoded oplog and the segments picked among
// them (host-staged batches; device-staged ones plan the same cuts in cut_kernel, dt_prep.hip).
#include "dt_cut.hpp"

#include <algorithm>
#include <set>

namespace dtgpu {

// Cut ranges [a, b] (every v in them is a cut), in LV order: at entry k ([s, t), parents P)
// the prefix's frontier minus P must be empty (then [0, v) is the version {v-1} for s < v <= t),
// and every later entry's parents must be >= v-1 (so each has v-1 in its history).
std::vector<std::pair<uint64_t, uint64_t>> cut_ranges(const SegInput &in) {
    const size_t ne = in.ent.size();
    std::vector<int64_t> sufmin(ne + 1, INT64_MAX);
    for (size_t k = ne; k-- > 0;) {
        int64_t mp = -1;   // ROOT
        if (in.poff[k + 1] > in.poff[k]) {
            mp = INT64_MAX;
            for (uint32_t j = in.poff[k]; j < in.poff[k + 1]; j++) mp = std::min<int64_t>(mp, int64_t(in.par[j]));
        }
        sufmin[k] = std::min(sufmin[k + 1], mp);
    }
    std::vector<std::pair<uint64_t, uint64_t>> cuts;
    std::set<uint64_t> F;   // frontier of the prefix
    for (size_t k = 0; k < ne; k++) {
        const uint64_t s = in.ent[k].first, t = in.ent[k].second;
        for (uint32_t j = in.poff[k]; j < in.poff[k + 1]; j++) F.erase(in.par[j]);
        if (F.empty()) {
            const int64_t lim = sufmin[k + 1] == INT64_MAX ? int64_t(t) : std::min<int64_t>(int64_t(t), sufmin[k + 1] + 1);
            if (lim >= int64_t(s) + 1) cuts.push_back({s + 1, uint64_t(lim)});
        }
        F.insert(t - 1);
    }
    return cuts;
}
std::vector<SegCut> plan_segments(const SegInput &in, const SegSettings &cfg) {
    std::vector<SegCut> out;
    const size_t ne = in.ent.size(), nop = in.ops.size();
    const uint32_t S = uint32_t(std::min<uint64_t>(cfg.max_seg, nop / cfg.ops_per_seg));
    if (S < 2 || ne == 0 || in.n_lv >= 0x7FFFFFFFull) return out;
    const std::vector<std::pair<uint64_t, uint64_t>> cuts = cut_ranges(in);
    if (cuts.empty()) return out;
    auto in_cut = [&](uint64_t v) {
        auto it = std::upper_bound(cuts.begin(), cuts.end(), std::make_pair(v, UINT64_MAX));
        return it != cuts.begin() && v <= std::prev(it)->second;
    };
    auto linear = [&](uint64_t lv, uint64_t len) {   // every op in [lv, lv+len) is concurrent with nothing
        auto it = std::upper_bound(cuts.begin(), cuts.end(), std::make_pair(lv, UINT64_MAX));
        return it != cuts.begin() && lv + len <= std::prev(it)->second;
    };
    // op-run starts that are cuts, nearest to the op runs where the cost reaches each equal share
    // (SegPlan::w_op, dt_prep.hpp); later cuts a quarter share of the cost past the previous one
    auto cost = [&](size_t j) { return uint64_t(cfg.w_op) * j + in.ops[j][0]; };
    const uint64_t total = uint64_t(cfg.w_op) * nop + in.ops[nop - 1][0] + in.ops[nop - 1][1], q4c = total / (4ull * S);
    std::vector<size_t> pick;
    for (uint32_t k = 1; k < S; k++) {
        const uint64_t tc = uint64_t(k) * total / S;
        size_t lo = 0, hi = nop;   // the first op run whose cost reaches tc
        while (lo < hi) {
            const size_t mid = (lo + hi) / 2;
            if (cost(mid) < tc) lo = mid + 1; else hi = mid;
        }
        const size_t target = lo;
        size_t best = SIZE_MAX;
        for (size_t d = 0; d < nop && best == SIZE_MAX; d++) {
            for (size_t j : {target - std::min(target, d), target + d}) {
                if (j > 0 && j < nop && in_cut(in.ops[j][0])) { best = j; break; }
            }
            if (d > nop / (2 * S)) break;   // no cut near this target
        }
        if (best != SIZE_MAX && (pick.empty() || cost(best) > cost(pick.back()) + q4c)) pick.push_back(best);
    }
    while (!pick.empty() && total - cost(pick.back()) < q4c) pick.pop_back();
    if (pick.empty()) return out;
    // prefix counts at the picked op runs
    int64_t ins = 0, del = 0, dconc = 0;
    size_t pi = 0;
    std::vector<std::array<int64_t, 3>> at(pick.size());
    uint64_t seg_ins = 0;
    std::vector<uint64_t> seg_ins_v;
    for (size_t j = 0; j <= nop; j++) {
        if (pi < pick.size() && j == pick[pi]) { at[pi++] = {ins, del, dconc}; seg_ins_v.push_back(seg_ins); seg_ins = 0; }
        if (j == nop) break;
        const auto &o = in.ops[j];
        if (o[2] == 0) { ins += int64_t(o[1]); seg_ins += o[1]; }
        else { del += int64_t(o[1]); if (!linear(o[0], o[1])) dconc += int64_t(o[1]); }
    }
    seg_ins_v.push_back(seg_ins);
    for (size_t k = 0; k <= pick.size(); k++) {
        SegCut c{};
        c.lo = k ? uint32_t(in.ops[pick[k - 1]][0]) : 0u;
        c.hi = k < pick.size() ? uint32_t(in.ops[pick[k]][0]) : 0xFFFFFFFFu;
        c.u = k ? uint32_t(std::max<int64_t>(0, std::min(at[k - 1][0], at[k - 1][0] - at[k - 1][1] + at[k - 1][2]))) : 0u;
        c.ins = seg_ins_v[k];
        out.push_back(c);
    }
    return out;
}

void seg_input_from_log(const HostOpLog &o, SegInput &si) {
    si.n_lv = o.n_lv;
    si.poff.push_back(0);
    for (const GraphEntry &g : o.graph.entries) {
        si.ent.push_back({g.start, g.end});
        for (uint64_t p : g.parents) si.par.push_back(p);
        si.poff.push_back(uint32_t(si.par.size()));
    }
    for (const OpRun &r : o.ops) si.ops.push_back({r.lv, r.len, uint64_t(r.kind)});
}

}  // namespace dtgpu
