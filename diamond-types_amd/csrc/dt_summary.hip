// dt_summary.hip -- batched version-summary intersection on MI355X (gfx950):
// CausalGraph::intersect_with_summary (src/causalgraph/summary.rs:175-264) up to find_dominators.
// One 64-lane wavefront per request; see dt_summary.hpp for the layout and the two launches.
//
// Resolve.  Every entry's name is matched against the document's agents, 64 agents per step: a lane
// compares the length, then the bytes (as add_doc matches a patch's agents).  Entry -> agent id is
// kept in the request's scratch; an unknown name (ROOT and over-long names among them) is NONE and
// its ranges come back whole.
//
// Sweep.  Range by range, in the summary's order, the document's agent runs go 64 per step: a lane
// whose run belongs to the range's agent clips it against the range, and the known pieces are
// compacted with ballots.  Going range by range re-reads the runs once per range (a hello names a
// handful of ranges; the runs of one document stay in L2), and in exchange the pieces of a range
// come out together and in LV order -- which is seq order unless older ops of the agent arrived in
// a later patch.
//
// Order.  A neighbour compare during the sweep tells whether a range's pieces ascend.  Only when
// they do not, the range's pieces are ranked by counting (runs of one agent never overlap in seq:
// the decoder defers documents where they do, so the ranks are unique) and put in order.
//
// Emit.  A piece's version is the LV of its last seq; it goes to the request's LV set as it is
// found (the mark sweep takes any order).  The gaps before, between and after the ordered pieces
// of a range are its remainder records, compacted with ballots.  The caller's extra LVs close the
// LV set.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dt_device.hpp"
#include "dt_mark.hpp"
#include "dt_summary.hpp"
#include "dt_wave.hpp"

namespace dtgpu {
namespace summ {
using namespace wave;
using hist::Base;
using hist::NONE;

// entry -> agent id of the document, by exact byte comparison of the names
DEV void resolve(const SumParams &P, const SumDesc &D, const Base &B, uint32_t n_agents, uint32_t in_len) {
    const uint32_t L = lane();
    uint32_t *eag = P.eag + D.eag_off;
    for (uint32_t i = 0; i < D.n_ent; i++) {
        const uint64_t n0 = P.name_off[D.ent0 + i], n1 = P.name_off[D.ent0 + i + 1];
        const uint8_t *name = P.names + n0;
        const uint64_t nlen = n1 - n0;
        uint32_t id = NONE;
        for (uint32_t a0 = 0; a0 < n_agents && id == NONE; a0 += 64) {
            const uint32_t a = a0 + L;
            const bool valid = a < n_agents;
            const uint32_t off = valid ? B.agents[2 * a] : 0, alen = valid ? B.agents[2 * a + 1] : 0;
            bool match = valid && uint64_t(alen) == nlen && uint64_t(off) + alen <= in_len;
            if (match)
                for (uint32_t k = 0; k < alen; k++)
                    if (B.in[off + k] != name[k]) { match = false; break; }
            const u64 m = ballot(match);
            if (m) id = a0 + ctz(m);
        }
        if (L == 0) eag[i] = id;
    }
    fence_agent();   // lane 0's words are read by every lane below
}

struct Range { uint64_t s, e; uint32_t ent, agent; };
DEV Range range_of(const SumParams &P, const SumDesc &D, uint32_t r) {
    Range R;
    R.s = P.ranges[2 * (D.rng0 + r)];
    R.e = P.ranges[2 * (D.rng0 + r) + 1];
    R.ent = P.range_ent[D.rng0 + r];
    R.agent = R.ent < D.n_ent ? P.eag[D.eag_off + R.ent] : NONE;
    return R;
}

// The known pieces of range R: the agent's runs clipped to it, in LV order.  EMIT: piece k of the
// range goes to pc[2 * k], its version to req[k] (both reserved for `room` pieces); `sorted` tells
// whether the pieces ascend in seq.  Returns the number of pieces.
template <bool EMIT>
DEV uint32_t sweep_range(const Base &B, uint32_t n_aruns, const Range &R, uint64_t *pc, uint32_t *req, uint32_t room,
                         bool &sorted) {
    uint32_t k = 0;
    uint64_t carry = 0;   // the end of the last piece so far
    sorted = true;
    for (uint32_t i0 = 0; i0 < n_aruns; i0 += 64) {
        const uint32_t i = i0 + lane();
        const bool v = i < n_aruns;
        const uint4 q = v ? reinterpret_cast<const uint4 *>(B.aruns)[i] : uint4{0, 0, 0, 0};   // lv, len, agent, seq
        const uint64_t rs = q.w, re = uint64_t(q.w) + q.y;
        const bool hit = v && q.z == R.agent && rs < R.e && re > R.s;
        const u64 m = ballot(hit);
        if (!m) continue;
        if (EMIT) {
            const uint64_t ps = rs > R.s ? rs : R.s, pe = re < R.e ? re : R.e;
            const u64 below = m & lt_mask();
            const uint32_t src = below ? last_lane(below) : 0;
            uint64_t prev = (uint64_t(shfl(uint32_t(pe >> 32), src)) << 32) | shfl(uint32_t(pe), src);
            if (!below) prev = carry;
            if (ballot(hit && ps < prev)) sorted = false;
            carry = rdl64(pe, last_lane(m));
            const uint32_t idx = k + bits_below(m);
            if (hit && idx < room) {
                pc[2 * size_t(idx)] = ps;
                pc[2 * size_t(idx) + 1] = pe;
                req[idx] = q.x + uint32_t(pe - 1 - rs);
            }
        }
        k += popc(m);
    }
    return k;
}

// Pieces pc[0, k) of one range in any order -> ascending seq, through tmp (k pairs): rank by counting.
DEV void order_pieces(uint64_t *pc, uint64_t *tmp, uint32_t k) {
    fence_agent();
    for (uint32_t j0 = 0; j0 < k; j0 += 64) {
        const uint32_t j = j0 + lane();
        const bool v = j < k;
        const uint64_t ps = v ? pc[2 * size_t(j)] : 0, pe = v ? pc[2 * size_t(j) + 1] : 0;
        uint32_t rank = 0;
        for (uint32_t t = 0; t < k; t++) rank += pc[2 * size_t(t)] < ps ? 1u : 0u;
        if (v) { tmp[2 * size_t(rank)] = ps; tmp[2 * size_t(rank) + 1] = pe; }
    }
    fence_agent();
    for (uint32_t j = lane(); j < 2 * k; j += 64) pc[j] = tmp[j];
}

// The uncovered stretches of range R around its ordered pieces pc[0, k): records (entry, start,
// end) appended at rem[3 * n_rem], room for c_rem records in all.  False when they do not fit.
DEV bool emit_gaps(const Range &R, const uint64_t *pc, uint32_t k, uint64_t *rem, uint32_t &n_rem, uint32_t c_rem) {
    bool fit = true;
    for (uint32_t j0 = 0; j0 <= k; j0 += 64) {   // candidate j: the gap before piece j (j == k: after the last)
        const uint32_t j = j0 + lane();
        const bool v = j <= k;
        const uint64_t gs = !v ? 0 : j == 0 ? R.s : pc[2 * size_t(j - 1) + 1];
        const uint64_t ge = !v ? 0 : j == k ? R.e : pc[2 * size_t(j)];
        const bool gap = v && gs < ge;
        const u64 m = ballot(gap);
        const uint32_t idx = n_rem + bits_below(m);
        if (gap && idx < c_rem) {
            rem[3 * size_t(idx)] = R.ent;
            rem[3 * size_t(idx) + 1] = gs;
            rem[3 * size_t(idx) + 2] = ge;
        }
        n_rem += popc(m);
        if (n_rem > c_rem) fit = false;
    }
    return fit;
}

__global__ __launch_bounds__(64) void sum_count_kernel(SumParams P) {
    const uint32_t doc = blockIdx.x;
    if (doc >= P.n_docs) return;
    const SumDesc D = P.docs[doc];
    const HistDesc HD = P.H.docs[doc];
    uint32_t st = D.skip, n_known = 0;
    if (!st) {
        const Base B = hist::base_of(P.H, HD);
        resolve(P, D, B, HD.b_n_agents, HD.b_in_len);
        for (uint32_t r = 0; r < D.n_rng; r++) {
            const Range R = range_of(P, D, r);
            if (R.s >= R.e) { st = hist::ErrArg; break; }
            if (R.agent == NONE) continue;
            bool sorted;
            const uint32_t k = sweep_range<false>(B, HD.b_n_aruns, R, nullptr, nullptr, 0, sorted);
            if (k > 0x7FFFFFFFu - n_known) { st = hist::ErrCapacity; break; }
            n_known += k;
        }
    }
    if (lane() == 0) {
        SumCounts &o = P.counts[doc];
        o.status = st; o.n_known = st ? 0u : n_known; o.n_rem = 0; o.n_resorted = 0;
    }
}

__global__ __launch_bounds__(64) void sum_emit_kernel(SumParams P, HistDesc *hdocs) {
    const uint32_t doc = blockIdx.x;
    if (doc >= P.n_docs) return;
    const SumDesc D = P.docs[doc];
    if (D.skip) return;   // the count launch's result stands
    const HistDesc HD = P.H.docs[doc];
    const Base B = hist::base_of(P.H, HD);
    uint64_t *pc = P.pieces + 2 * D.pc_off, *rem = P.rem + 3 * D.rem_off;
    uint32_t *req = P.req + HD.req_off;
    uint32_t st = 0, n_known = 0, n_rem = 0, n_resorted = 0;
    for (uint32_t r = 0; r < D.n_rng && !st; r++) {
        const Range R = range_of(P, D, r);
        uint32_t k = 0;
        if (R.agent != NONE) {
            bool sorted;
            k = sweep_range<true>(B, HD.b_n_aruns, R, pc + 2 * size_t(n_known), req + n_known, D.c_known - n_known, sorted);
            if (k > D.c_known - n_known) { st = hist::ErrCapacity; break; }
            if (!sorted) {
                order_pieces(pc + 2 * size_t(n_known), pc + 2 * size_t(D.c_known), k);
                n_resorted++;
            }
            fence_agent();   // the pieces are read back by other lanes
        }
        if (!emit_gaps(R, pc + 2 * size_t(n_known), k, rem, n_rem, D.c_rem)) st = hist::ErrCapacity;
        n_known += k;
    }
    if (!st && n_known != D.c_known) st = hist::ErrCapacity;   // the two launches disagree
    if (!st)
        for (uint32_t j = lane(); j < D.n_ext; j += 64) req[n_known + j] = P.ext[D.ext_off + j];
    if (lane() == 0) {
        SumCounts &o = P.counts[doc];
        o.status = st; o.n_known = st ? 0u : n_known; o.n_rem = st ? 0u : n_rem; o.n_resorted = n_resorted;
        if (st) hdocs[doc].skip = st;   // the mark launch that follows reports it
    }
}

}  // namespace summ

int launch_sum_count(const SumParams &p, void *stream) {
    if (!p.n_docs) return 0;
    hipLaunchKernelGGL(summ::sum_count_kernel, dim3(p.n_docs), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), p);
    return launch_error() == hipSuccess ? 0 : 66;
}

int launch_sum_emit(const SumParams &p, void *stream) {
    if (!p.n_docs) return 0;
    hipLaunchKernelGGL(summ::sum_emit_kernel, dim3(p.n_docs), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), p,
                       const_cast<HistDesc *>(p.H.docs));
    return launch_error() == hipSuccess ? 0 : 66;
}

}  // namespace dtgpu
