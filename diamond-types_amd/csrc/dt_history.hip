// dt_history.hip -- batched history projection on MI355X (gfx950): ListOpLog::checkout(&[LV])
// (src/list/oplog.rs:32-36) up to the replay.  One 64-lane wavefront per output builds the history
// of a version of a resident document as an oplog of its own; see dt_history.hpp for the layout.
//
// Mark (hist_mark_kernel).  Hist(version) holds a prefix of every graph entry, so one word per
// entry describes it.  The word is the maximum over (x + 1) << 1 | from_edge of the LVs x known to
// be in the history: seeded from the request, then swept from the highest entry down, 64 entries
// per step, every included entry pushing its parents with an atomic max (parents lie below their
// entry, so only pushes inside the step need the repeat-until-stable loop).  A request LV that
// still ends its entry's prefix with the edge bit clear is a dominator: the reduced frontier
// falls out of the same sweep, ascending.  An exclusive scan of the prefix lengths gives each
// entry's new base LV.
//
// Emit (hist_emit_kernel).  The host's rules (dtgpu_api.cpp history_oplog / copy_clipped over
// HostOpLog::assign, push_ins, push_del, Graph::push and finish), restated for 64 lanes: every
// stream first writes its clipped pieces compacted into the output arena itself, then a merge
// pass over the pieces decides the run heads in place.  Whether a piece continues its predecessor
// is a property of the two pieces alone, except for delete runs, whose direction is fixed by the
// run's second piece: there the heads of a step come from its ballots and a scalar loop over the
// (rare) direction changes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dt_device.hpp"
#include "dt_history.hpp"
#include "dt_mark.hpp"
#include "dt_wave.hpp"

namespace dtgpu {
namespace hist {
using namespace wave;

// (field by field: a whole-struct copy would keep the result in scratch memory)
__device__ __forceinline__ void write_result(DecodeResult &o, uint32_t st, const Counts &R, uint32_t n_agents, uint32_t form) {
    o.status = st;
    o.n_file_agents = 0; o.n_agents = st ? 0u : n_agents; o.n_aruns = R.n_aruns; o.n_pre = 0; o.n_ops = R.n_ops;
    o.n_entries = R.n_entries; o.n_parents = R.n_parents; o.n_content = R.n_content; o.n_version = R.n_version;
    o.content_complete = R.complete; o.ascii = R.ascii; o.n_lv = R.n_lv;
    o.lz_len = 0; o.tp_bytes = 0; o.cik_bytes = 0; o.hist_bytes = 0; o.raw_aruns = 0; o.n_file_frontier = 0;
    o.prof[0] = form;
    for (int k = 1; k < 8; k++) o.prof[k] = 0;
    o.doc_id_off = 0; o.doc_id_len = NONE;
}

__global__ __launch_bounds__(64) void hist_mark_kernel(HistParams P) {
    extern __shared__ uint32_t lds[];
    const uint32_t doc = blockIdx.x;
    if (doc >= P.n_docs) return;
    const HistDesc D = P.docs[doc];
    Counts R{};
    uint32_t st = D.skip;
    if (!st) st = mark_doc(P, D, lds, R);
    if (st) R = Counts{};
    if (lane() == 0) write_result(P.results[doc], st, R, D.b_n_agents, D.skip ? 0u : D.use_lds ? 1u : 2u);
}

// ---- emit ------------------------------------------------------------------------------------
struct Out {
    uint32_t *aruns, *ops, *ent, *poff, *par, *cbyte, *agents;
    uint8_t *content, *in;
};

// Graph entries: an included entry starts a new entry unless its only (mapped) parent is the
// previous new LV (Graph::push); parents mapped in order (the map is monotone).  keep: every
// included entry stays an entry of its own (HistParams::keep_entries).
__device__ __forceinline__ bool emit_entries(const HistDesc &D, const Base &B, const Scr &S, const Out &O, uint32_t n_lv,
                                             uint32_t &n_ent, uint32_t &n_par, bool keep) {
    const uint32_t L = lane();
    uint32_t nh = 0, np_tot = 0;
    bool over = false;
    for (uint32_t e0 = 0; e0 < B.ne; e0 += 64) {
        const uint32_t e = e0 + L;
        const bool valid = e < B.ne;
        const uint32_t st = valid ? B.ent[2 * e] : 0, r = valid ? S.reach[e] : 0;
        const bool inc = valid && r > st;
        const uint32_t nbv = inc ? S.nb[e] : 0;
        const uint32_t p0 = inc ? B.poff[e] : 0, np = inc ? B.poff[e + 1] - p0 : 0;
        const uint32_t m0 = np ? map_lv(B, S, B.par[p0]) : NONE;
        const bool head = inc && (keep || !(np == 1 && m0 + 1 == nbv));
        if (valid) S.head[e] = head ? 1u : 0u;
        const uint64_t hm = ballot(head);
        const uint32_t k = nh + popc(hm & lt_mask());
        const uint32_t pc = head ? np : 0, pin = scan_incl(pc), pofs = np_tot + pin - pc;
        if (head) {
            if (k < D.c_ent && pofs + np <= D.c_par) {
                O.ent[2 * k] = nbv;
                if (k) O.ent[2 * k - 1] = nbv;
                O.poff[k] = pofs;
                for (uint32_t t = 0; t < np; t++) O.par[pofs + t] = t ? map_lv(B, S, B.par[p0 + t]) : m0;
            } else {
                over = true;
            }
        }
        nh += popc(hm);
        np_tot += rdl(pin, 63);
    }
    if (ballot(over)) return false;
    if (L == 0) {
        if (nh) O.ent[2 * nh - 1] = n_lv;
        O.poff[nh] = np_tot;
    }
    n_ent = nh; n_par = np_tot;
    return true;
}

// Agent runs clipped to the included entry prefixes, compacted into O.aruns as (new LV, len,
// agent, seq); returns the piece count, or NONE when the arena is too small.
__device__ __forceinline__ uint32_t arun_pieces(const HistDesc &D, const Base &B, const Scr &S, const Out &O) {
    const uint32_t L = lane();
    uint32_t total = 0;
    bool over = false;
    for (uint32_t e0 = 0; e0 < B.ne; e0 += 64) {
        const uint32_t e = e0 + L;
        const bool valid = e < B.ne;
        const uint32_t st = valid ? B.ent[2 * e] : 0, r = valid ? S.reach[e] : 0;
        const bool inc = valid && r > st;
        const uint32_t a0 = inc ? find_le(B.aruns, 4, D.b_n_aruns, st) : 0;
        const uint32_t a1 = inc ? find_le(B.aruns, 4, D.b_n_aruns, r - 1) : 0;
        const uint32_t cnt = inc ? a1 - a0 + 1 : 0, incl = scan_incl(cnt), off = total + incl - cnt;
        if (inc) {
            const uint32_t nbv = S.nb[e];
            if (off + cnt <= D.c_arun) {
                for (uint32_t a = a0; a <= a1; a++) {
                    const uint4 A = reinterpret_cast<const uint4 *>(B.aruns)[a];
                    const uint32_t x = umax(A.x, st), y = umin(A.x + A.y, r);
                    reinterpret_cast<uint4 *>(O.aruns)[off + (a - a0)] = uint4{nbv + (x - st), y - x, A.z, A.w + (x - A.x)};
                }
            } else {
                over = true;
            }
        }
        total += rdl(incl, 63);
    }
    return ballot(over) ? NONE : total;
}

struct OpTotals { uint32_t n_pieces, n_bytes, n_known, unknown; };

// Op runs clipped to their entry's prefix (a reverse delete run from the right), compacted into
// O.ops as (new LV, len, pos, kind | fwd << 1 | starts a new entry << 2); each entry's content
// delta (new byte offset - old byte offset of its known chars).
__device__ __forceinline__ bool op_pieces(const HistDesc &D, const Base &B, const Scr &S, const Out &O, OpTotals &T) {
    const uint32_t L = lane();
    uint32_t cnt = 0, cb = 0, known = 0;
    bool over = false, unk = false;
    for (uint32_t i0 = 0; i0 < D.b_n_ops; i0 += 64) {
        const uint32_t i = i0 + L;
        const bool v = i < D.b_n_ops;
        const uint4 q = v ? reinterpret_cast<const uint4 *>(B.ops)[i] : uint4{0, 0, 0, 0};
        const uint32_t e = v ? entry_of(B, q.x) : 0;
        const uint32_t st = v ? B.ent[2 * e] : 0, r = v ? S.reach[e] : 0;
        const bool inc = v && q.x < r;
        const uint32_t y = umin(q.x + q.y, r), len = y - q.x;
        const bool del = q.w & 1u, fwd = (q.w >> 1) & 1u;
        const uint32_t pos = (del && !fwd) ? q.z + (q.x + q.y - y) : q.z;
        uint32_t b0 = 0, b1 = 0, nk = 0;
        if (inc && !del) {
            nk = piece_bytes(B, D.b_complete != 0, q.x, y, b0, b1);
            if (nk < len) unk = true;
        }
        const uint32_t nb = b1 - b0, bincl = scan_incl(nb), dst = cb + bincl - nb;
        if (nk) S.delta[e] = dst - b0;
        const uint64_t im = ballot(inc);
        const uint32_t k = cnt + popc(im & lt_mask());
        if (inc) {
            if (k < D.c_op) {
                const uint32_t es = (q.x == st && S.head[e]) ? 4u : 0u;
                reinterpret_cast<uint4 *>(O.ops)[k] = uint4{S.nb[e] + (q.x - st), len, pos, (q.w & 3u) | es};
            } else {
                over = true;
            }
        }
        cnt += popc(im);
        cb += rdl(bincl, 63);
        known += wave_sum(nk);
    }
    T.n_pieces = cnt; T.n_bytes = cb; T.n_known = known; T.unknown = ballot(unk) ? 1u : 0u;
    return !ballot(over);
}

// link of piece q to its predecessor p: 0 none, 1 insert / agent run continues, 2 delete forward,
// 3 delete backward (HostOpLog::assign, push_ins, push_del)
template <bool OPS>
__device__ __forceinline__ uint32_t link_of(const uint4 &p, const uint4 &q) {
    if (!OPS) return (p.z == q.z && p.w + p.y == q.w) ? 1u : 0u;
    const uint32_t kp = p.w & 1u, kq = q.w & 1u;
    if (kp != kq) return 0;
    if (!kq) return p.z + p.y == q.z ? 1u : 0u;
    const bool fp = (p.w >> 1) & 1u, fq = (q.w >> 1) & 1u;
    if ((p.y == 1 || fp) && (q.y == 1 || fq) && q.z == p.z) return 2;
    if ((p.y == 1 || !fp) && (q.y == 1 || !fq) && q.z + q.y == p.z) return 3;
    return 0;
}

// The merge pass over n compacted pieces in `arr` (quads), in place: run heads by the RLE rules
// (for op runs then split again where a new graph entry starts, HostOpLog::finish).  A head
// writes its run's first LV and kind (agent, seq); the run's last piece writes the length and,
// for op runs, the position (of the first LV of an insert or forward delete run, of the last
// piece of a backward delete run).  Returns the run count.
template <bool OPS>
__device__ __forceinline__ uint32_t merge_pass(uint32_t *arr, uint32_t n) {
    const uint32_t L = lane();
    const uint4 *in = reinterpret_cast<const uint4 *>(arr);
    uint4 cq{0, 0, 0, 0};          // the previous step's last piece
    uint32_t ct = 0, cmh = 1;      // its link and whether it heads its run
    uint32_t chead = 0, nout = 0;  // first LV + 1 of the open run, runs so far
    for (uint32_t s = 0; s < n; s += 64) {
        const uint32_t i = s + L;
        const bool v = i < n;
        const uint4 q = v ? in[i] : uint4{0, 0, 0, 0};
        const bool ext = s + 64 < n;
        const uint4 nq = ext ? in[s + 64] : uint4{0, 0, 0, 0};
        uint4 p;
        p.x = __shfl_up(q.x, 1, 64); p.y = __shfl_up(q.y, 1, 64); p.z = __shfl_up(q.z, 1, 64); p.w = __shfl_up(q.w, 1, 64);
        if (L == 0) p = cq;
        const uint32_t t = (v && i > 0) ? link_of<OPS>(p, q) : 0u;
        uint32_t pt = __shfl_up(t, 1, 64);
        if (L == 0) pt = ct;
        uint64_t mhm = ballot(v && t == 0);
        if (OPS) {
            uint64_t cm = ballot(v && t != 0 && t != pt);
            while (cm) {
                const uint32_t b = uint32_t(__ffsll((unsigned long long)cm) - 1);
                cm &= cm - 1;
                const bool pmh = b ? (mhm >> (b - 1)) & 1ull : cmh != 0;
                if (!pmh) mhm |= 1ull << b;
            }
        }
        const bool mh = (mhm >> L) & 1ull;
        const bool fh = v && (mh || (OPS && (q.w & 4u)));
        // the successor's link, and whether it heads a run / a final run
        uint32_t tn = __shfl_down(t, 1, 64);
        bool mhn = __shfl_down(uint32_t(mh), 1, 64) != 0, fhn = __shfl_down(uint32_t(fh), 1, 64) != 0;
        if (L == 63) {
            tn = ext ? link_of<OPS>(q, nq) : 0u;
            mhn = tn == 0 || (OPS && tn != t && !mh);
            fhn = mhn || (OPS && (nq.w & 4u));
        }
        if (i + 1 >= n) { tn = 0; mhn = true; fhn = true; }
        const uint32_t hl = umax(scan_max(fh ? q.x + 1 : 0u), chead);
        const uint64_t fm = ballot(fh);
        const uint32_t k = nout + popc(fm & (lt_mask() | (1ull << L))) - 1;
        if (fh) {
            arr[4 * k] = q.x;
            if (OPS) {
                uint32_t f = (q.w >> 1) & 1u;
                if (q.w & 1u) {   // a delete run of two or more pieces has the direction of its links
                    const uint32_t d = !mh ? t : !mhn ? tn : 0u;
                    if (d) f = d == 2 ? 1u : 0u;
                }
                arr[4 * k + 3] = (q.w & 1u) | (f << 1);
            } else {
                arr[4 * k + 2] = q.z;
                arr[4 * k + 3] = q.w;
            }
        }
        if (v && fhn) {
            const uint32_t h = hl - 1;
            arr[4 * k + 1] = q.x + q.y - h;
            if (OPS) arr[4 * k + 2] = (q.w & 1u) ? q.z : q.z - (q.x - h);
        }
        cq.x = rdl(q.x, 63); cq.y = rdl(q.y, 63); cq.z = rdl(q.z, 63); cq.w = rdl(q.w, 63);
        ct = rdl(t, 63); cmh = rdl(uint32_t(mh), 63);
        chead = rdl(hl, 63);
        nout += popc(fm);
    }
    return nout;
}

// Per-LV content offsets and the kept inserts' bytes: 64 new LVs per step, each lane finding its
// entry among the next 64 entries' new base LVs (a merge path: a step covers 64 LVs or 64 entries).
__device__ __forceinline__ bool fill_lvs(const HistDesc &D, const Base &B, const Scr &S, const Out &O, uint32_t n_lv) {
    const uint32_t L = lane();
    uint32_t j0 = 0, ec = 0;
    bool over = false;
    while (j0 < n_lv) {
        const uint32_t ew = ec + L;
        const uint32_t nbv = ew < B.ne ? S.nb[ew] : NONE;
        const uint32_t nb_next = ec + 64 < B.ne ? S.nb[ec + 64] : n_lv;
        const uint32_t jlim = umin(j0 + 64, nb_next);
        if (jlim == j0) { ec += 64; continue; }   // 64 entries outside the history
        const uint32_t j = j0 + L;
        const bool act = j < jlim;
        uint32_t k = 0;   // the last window entry with a base <= j (bases ascend; the window's first is <= j0)
        for (uint32_t step = 32; step; step >>= 1) {
            const uint32_t cand = k + step;
            const uint32_t val = __shfl(nbv, cand & 63u, 64);
            if (cand < 64 && val <= j) k = cand;
        }
        const uint32_t e = ec + k;
        if (act) {
            const uint32_t src = B.ent[2 * e] + (j - S.nb[e]);
            const uint32_t c = B.cbyte[src];
            uint32_t o = NONE;
            if (c != NONE) {
                o = c + S.delta[e];
                const uint32_t nbt = utf8_len(B.content[c]);
                if (o + nbt <= D.c_content) {
                    for (uint32_t t = 0; t < nbt; t++) O.content[o + t] = B.content[c + t];
                } else {
                    over = true;
                }
            }
            O.cbyte[j] = o;
        }
        ec = rdl(e, jlim - j0 - 1);
        j0 = jlim;
    }
    return !ballot(over);
}

// Every agent name, packed into the output's `in` region; (offset, length) pairs rewritten to it.
__device__ __forceinline__ bool copy_names(const HistDesc &D, const Base &B, const Out &O) {
    const uint32_t L = lane();
    uint32_t total = 0;
    bool over = false;
    for (uint32_t a0 = 0; a0 < D.b_n_agents; a0 += 64) {
        const uint32_t a = a0 + L;
        const bool v = a < D.b_n_agents;
        const uint32_t off = v ? B.agents[2 * a] : 0, len = v ? B.agents[2 * a + 1] : 0;
        const uint32_t incl = scan_incl(len), dst = total + incl - len;
        if (v) {
            if (a < D.c_agent && dst + len <= D.c_in) {
                O.agents[2 * a] = dst;
                O.agents[2 * a + 1] = len;
                for (uint32_t t = 0; t < len; t++) O.in[dst + t] = B.in[off + t];
            } else {
                over = true;
            }
        }
        total += rdl(incl, 63);
    }
    return !ballot(over);
}

__device__ __forceinline__ uint32_t emit_doc(const HistParams &P, const HistDesc &D, Counts &R) {
    const Base B = base_of(P, D);
    const Scr S = scr_of(P, D);
    Out O;
    O.aruns = P.o_aruns + 4 * D.o_arun; O.ops = P.o_ops + 4 * D.o_op; O.ent = P.o_ent + 2 * D.o_ent;
    O.poff = P.o_poff + D.o_poff; O.par = P.o_par + D.o_par; O.cbyte = P.o_cbyte + D.o_lv;
    O.agents = P.o_agents + 2 * D.o_agent; O.content = P.o_content + D.o_content; O.in = P.o_in + D.o_in;
    const uint32_t n_lv = R.n_lv;
    if (n_lv > D.c_lv) return ErrCapacity;
    uint32_t n_ent = 0, n_par = 0;
    if (!emit_entries(D, B, S, O, n_lv, n_ent, n_par, P.keep_entries != 0)) return ErrCapacity;
    const uint32_t apieces = arun_pieces(D, B, S, O);
    if (apieces == NONE) return ErrCapacity;
    fence_agent();   // the pieces and the entry heads, before the passes that read them
    const uint32_t n_aruns = merge_pass<false>(O.aruns, apieces);
    OpTotals T;
    if (!op_pieces(D, B, S, O, T)) return ErrCapacity;
    fence_agent();
    const uint32_t n_ops = merge_pass<true>(O.ops, T.n_pieces);
    if (T.n_bytes > D.c_content) return ErrCapacity;
    if (!fill_lvs(D, B, S, O, n_lv)) return ErrCapacity;
    if (!copy_names(D, B, O)) return ErrCapacity;
    R.n_entries = n_ent; R.n_parents = n_par; R.n_aruns = n_aruns; R.n_ops = n_ops;
    R.n_content = T.n_bytes; R.complete = T.unknown ? 0u : 1u; R.ascii = T.n_bytes == T.n_known ? 1u : 0u;
    return S_OK;
}

__global__ __launch_bounds__(64) void hist_emit_kernel(HistParams P) {
    const uint32_t doc = blockIdx.x;
    if (doc >= P.n_docs) return;
    const HistDesc D = P.docs[doc];
    if (D.skip) return;   // the mark launch's result stands
    Counts R{};
    R.n_lv = uint32_t(P.results[doc].n_lv);
    R.n_version = P.results[doc].n_version;
    const uint32_t form = P.results[doc].prof[0];
    const uint32_t st = emit_doc(P, D, R);
    if (st) R = Counts{};
    if (lane() == 0) write_result(P.results[doc], st, R, D.b_n_agents, form);
}

}  // namespace hist

int launch_hist_mark(const HistParams &p, void *stream) {
    if (!p.n_docs) return 0;
    if (p.lds_entries > HIST_LDS_ENTRIES) return 65;
    hipLaunchKernelGGL(hist::hist_mark_kernel, dim3(p.n_docs), dim3(64), size_t(p.lds_entries) * 4,
                       reinterpret_cast<hipStream_t>(stream), p);
    return launch_error() == hipSuccess ? 0 : 66;
}

int launch_hist_emit(const HistParams &p, void *stream) {
    if (!p.n_docs) return 0;
    hipLaunchKernelGGL(hist::hist_emit_kernel, dim3(p.n_docs), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), p);
    return launch_error() == hipSuccess ? 0 : 66;
}

}  // namespace dtgpu
