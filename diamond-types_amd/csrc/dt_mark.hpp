// dt_mark.hpp -- the history mark sweep, shared by the history projection (dt_history.hip) and the
// patch encoder (dt_patch.hip).
//
// Hist(version) holds a prefix of every graph entry, so one word per entry describes it.  The word
// is the maximum over (x + 1) << 1 | from_edge of the LVs x known to be in the history: seeded from
// the request, then swept from the highest entry down, 64 entries per step, every included entry
// pushing its parents with an atomic max (parents lie below their entry, so only pushes inside the
// step need the repeat-until-stable loop).  A request LV that still ends its entry's prefix with
// the edge bit clear is a dominator: the reduced frontier falls out of the same sweep, ascending.
// mark_doc leaves reach[e] (the end of entry e's prefix, 0: not in the history) and the new base LV
// of every entry in the request's scratch, and counts what the history needs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dt_device.hpp"
#include "dt_history.hpp"
#include "dt_wave.hpp"

namespace dtgpu {
namespace hist {
using namespace wave;

enum : uint32_t { S_OK = 0, ErrCapacity = 65, ErrArg = 67, Defer = DECODE_DEFER };
constexpr uint32_t NONE = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }

// The last index i < n with a[i * stride] <= key (a ascending, a[0] <= key, n >= 1).
__device__ __forceinline__ uint32_t find_le(const uint32_t *a, uint32_t stride, uint32_t n, uint32_t key) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a[size_t(mid) * stride] <= key) lo = mid; else hi = mid;
    }
    return lo;
}

struct Base {                // the resident document's arrays
    const uint32_t *ent;     // pairs
    const uint32_t *poff, *par, *aruns, *ops, *cbyte, *agents;
    const uint8_t *content, *in;
    uint32_t ne;
};
struct Scr { uint32_t *reach, *nb, *delta, *head; };

__device__ __forceinline__ Base base_of(const HistParams &P, const HistDesc &D) {
    Base B;
    B.ent = P.b_ent + 2 * D.b_ent; B.poff = P.b_poff + D.b_poff; B.par = P.b_par + D.b_par;
    B.aruns = P.b_aruns + 4 * D.b_arun; B.ops = P.b_ops + 4 * D.b_op; B.cbyte = P.b_cbyte + D.b_lv;
    B.agents = P.b_agents + 2 * D.b_agent; B.content = P.b_content + D.b_content; B.in = P.b_in + D.b_in;
    B.ne = D.b_n_ent;
    return B;
}
__device__ __forceinline__ Scr scr_of(const HistParams &P, const HistDesc &D) {
    Scr S;
    S.reach = P.scr + D.scr_off; S.nb = S.reach + D.b_n_ent; S.delta = S.nb + D.b_n_ent; S.head = S.delta + D.b_n_ent;
    return S;
}
__device__ __forceinline__ uint32_t entry_of(const Base &B, uint32_t lv) { return find_le(B.ent, 2, B.ne, lv); }
// old LV (inside the history) -> new LV
__device__ __forceinline__ uint32_t map_lv(const Base &B, const Scr &S, uint32_t lv) {
    const uint32_t e = entry_of(B, lv);
    return S.nb[e] + (lv - B.ent[2 * e]);
}

// The content bytes [b0, b1) of the known chars of the insert LVs [x, y), and how many are known.
__device__ __forceinline__ uint32_t piece_bytes(const Base &B, bool complete, uint32_t x, uint32_t y, uint32_t &b0, uint32_t &b1) {
    b0 = b1 = 0;
    if (complete) {   // every insert is known: the first and the last char bound the bytes
        b0 = B.cbyte[x];
        const uint32_t l = B.cbyte[y - 1];
        if (b0 != NONE && l != NONE) {
            b1 = l + utf8_len(B.content[l]);
            return y - x;
        }
        b0 = 0;
    }
    uint32_t nk = 0, last = 0;
    for (uint32_t u = x; u < y; u++) {
        const uint32_t c = B.cbyte[u];
        if (c == NONE) continue;
        if (!nk) b0 = c;
        last = c;
        nk++;
    }
    if (nk) b1 = last + utf8_len(B.content[last]);
    return nk;
}

// ---- mark ----------------------------------------------------------------------------------
struct Counts { uint32_t n_lv, n_version, n_entries, n_parents, n_aruns, n_ops, n_content, complete, ascii; };

__device__ __forceinline__ uint32_t mark_doc(const HistParams &P, const HistDesc &D, uint32_t *lds, Counts &R) {
    const Base B = base_of(P, D);
    const Scr S = scr_of(P, D);
    const uint32_t ne = B.ne, L = lane();
    if (D.b_n_lv >= 0x7FFFFFFEu) return Defer;   // (x + 1) << 1 must fit the mark word
    uint32_t *W = D.use_lds ? lds : S.reach;
    for (uint32_t i = L; i < ne; i += 64) W[i] = 0;
    fence_agent();
    {   // seed
        const uint32_t *req = P.req + D.req_off;
        bool bad = false;
        for (uint32_t i = L; i < D.n_req; i += 64) {
            const uint32_t v = req[i];
            if (v >= D.b_n_lv) { bad = true; continue; }
            atomicMax(&W[entry_of(B, v)], (v + 1) << 1);
        }
        if (ballot(bad)) return ErrArg;
    }
    for (int64_t hi = ne; hi > 0; hi -= 64) {   // entries [hi - 64, hi), highest first
        const int64_t es = hi - 1 - int64_t(L);
        const bool valid = es >= 0;
        const uint32_t e = valid ? uint32_t(es) : 0;
        bool pushed = false;
        for (;;) {
            // words in LDS: the wave's own pushes only have to complete (the base arrays read here
            // are never written, so their L1 lines stay); in HBM the atomics went to L2.  (use_lds
            // == 2 keeps the agent-scope fence with the words in LDS: the A/B of the bench tools.)
            if (D.use_lds == 1) fence_workgroup(); else fence_agent();
            const uint32_t w = valid ? __hip_atomic_load(&W[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
            const bool go = valid && w != 0 && !pushed;
            if (!ballot(go)) break;
            if (go) {
                const uint32_t p1 = B.poff[e + 1];
                for (uint32_t k = B.poff[e]; k < p1; k++) {
                    const uint32_t p = B.par[k];
                    atomicMax(&W[entry_of(B, p)], ((p + 1) << 1) | 1u);
                }
                pushed = true;
            }
        }
    }
    fence_agent();
    // prefix ends, the LV map, the reduced frontier, bounds of entries / parents / agent runs
    uint32_t total = 0, nfront = 0, n_ent = 0, n_par = 0, n_ar = 0;
    uint32_t *front = P.o_front + D.o_ver, *ver = P.o_ver + D.o_ver;
    for (uint32_t e0 = 0; e0 < ne; e0 += 64) {
        const uint32_t e = e0 + L;
        const bool valid = e < ne;
        const uint32_t w = valid ? __hip_atomic_load(&W[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        const uint32_t r = w >> 1, st = valid ? B.ent[2 * e] : 0;
        const bool inc = w != 0;
        const uint32_t len = inc ? r - st : 0;
        const uint32_t incl = scan_incl(len), nbv = total + incl - len;
        if (valid) { S.reach[e] = r; S.nb[e] = nbv; }
        const bool isf = inc && !(w & 1u);
        const uint64_t fm = ballot(isf);
        const uint32_t fi = nfront + popc(fm & lt_mask());
        if (isf && fi < DECODE_MAX_FRONTIER) { front[fi] = r - 1; ver[fi] = nbv + len - 1; }
        nfront += popc(fm);
        total += rdl(incl, 63);
        n_ent += popc(ballot(inc));
        n_par += wave_sum(inc ? B.poff[e + 1] - B.poff[e] : 0);
        n_ar += wave_sum(inc ? find_le(B.aruns, 4, D.b_n_aruns, r - 1) - find_le(B.aruns, 4, D.b_n_aruns, st) + 1 : 0);
    }
    if (nfront > DECODE_MAX_FRONTIER) return Defer;
    fence_agent();
    // op runs that intersect the history, their content bytes
    uint32_t n_op = 0, n_bytes = 0;
    for (uint32_t i0 = 0; i0 < D.b_n_ops; i0 += 64) {
        const uint32_t i = i0 + L;
        const bool v = i < D.b_n_ops;
        const uint4 q = v ? reinterpret_cast<const uint4 *>(B.ops)[i] : uint4{0, 0, 0, 0};
        const uint32_t e = v ? entry_of(B, q.x) : 0;
        const uint32_t r = v ? S.reach[e] : 0;
        const bool inc = v && q.x < r;
        uint32_t b0 = 0, b1 = 0;
        if (inc && !(q.w & 1u)) piece_bytes(B, D.b_complete != 0, q.x, umin(q.x + q.y, r), b0, b1);
        n_op += popc(ballot(inc));
        n_bytes += wave_sum(b1 - b0);
    }
    R.n_lv = total; R.n_version = nfront; R.n_entries = n_ent; R.n_parents = n_par; R.n_aruns = n_ar;
    R.n_ops = n_op; R.n_content = n_bytes;
    return S_OK;
}

}  // namespace hist
}  // namespace dtgpu
