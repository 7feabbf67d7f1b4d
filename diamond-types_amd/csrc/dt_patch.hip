// dt_patch.hip -- batched patch encoder on MI355X (gfx950): ListOpLog::encode_from(opts, from)
// (src/list/encoding/encode_oplog.rs:404-747), one 64-lane wavefront per request; see dt_patch.hpp.
// The host encoder (dt_encode.cpp encode_dt) is the byte-exact specification.
//
// Mark (patch_mark_kernel).  The history mark sweep of dt_mark.hpp leaves reach[e], the end of
// entry e's prefix inside Hist(from); the new ops of e are [max(reach[e], start), end).  One more
// pass over the entries and the op runs counts the patch.
//
// Build (patch_build_kernel).
//   A  pieces     the entries with new ops, compacted in ascending LV order; a piece that starts
//                 inside its entry has the single parent start - 1 (clone_parents_at_version)
//   B  edges      only parents inside the patch: children CSR (counts and slots by atomics, each
//                 list then sorted ascending), a pending-parents counter per piece
//   C  walk       SpanningTreeWalker (txn_trace.rs:114-333; spanning_walk in dt_host.cpp): the
//                 stack starts with the parentless pieces reversed; a merge on top (two or more
//                 parents in the graph, inside the patch or not) yields to the nearest non-merge
//                 below it; a visited piece pushes its children whose parents are all visited.
//                 Wave-uniform, the stack search and the pushes 64 lanes wide.
//   D  records    one wave-uniform loop over the walk steps keeps the agent map in the host's
//                 order of first mention (a step's agent runs, then the foreign parents of the txn
//                 that step closes; after the walk the last txn's, then the StartBranch version)
//                 and writes the agent assignment and txn streams; op-run pieces are gathered lane-
//                 parallel in walk order and merged by can_append / append in registers
//   E  bytes      sizes by prefix sums, text gather, LZ4, chunk headers, records serialised lane-
//                 parallel at their final offsets, CRC-32C (dt_enc_dev.hpp, shared with dt_encoder.hip)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dt_device.hpp"
#include "dt_enc_dev.hpp"
#include "dt_mark.hpp"
#include "dt_patch.hpp"
#include "dt_wave.hpp"

namespace dtgpu {
namespace patch {
using namespace wave;
using enc::leb_len;
using enc::put_leb;
using enc::zz_old;
using hist::Base;
using hist::Scr;
using hist::NONE;
using hist::find_le;
using hist::umax;
using hist::umin;

enum : uint32_t { S_OK = 0, ErrCheckout = 64, ErrCapacity = 65 };

// a scratch word another lane of this wave may have written since the last fence
DEV uint32_t ldw(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// ---- mark ------------------------------------------------------------------------------------
DEV void count_patch(const HistParams &P, const HistDesc &D, PatchCounts &C) {
    const Base B = hist::base_of(P, D);
    const Scr S = hist::scr_of(P, D);
    const uint32_t L = lane();
    uint32_t np = 0, nlv = 0, npar = 0, nar = 0, nop = 0, ntext = 0;
    for (uint32_t e0 = 0; e0 < B.ne; e0 += 64) {
        const uint32_t e = e0 + L;
        const bool valid = e < B.ne;
        const uint32_t st = valid ? B.ent[2 * e] : 0, en = valid ? B.ent[2 * e + 1] : 0;
        const uint32_t ps = umax(valid ? S.reach[e] : 0, st);
        const bool pc = valid && ps < en;
        np += popc(ballot(pc));
        nlv += wave_sum(pc ? en - ps : 0);
        npar += wave_sum(pc ? (ps > st ? 1u : B.poff[e + 1] - B.poff[e]) : 0);
        nar += wave_sum(pc ? find_le(B.aruns, 4, D.b_n_aruns, en - 1) - find_le(B.aruns, 4, D.b_n_aruns, ps) + 1 : 0);
    }
    for (uint32_t i0 = 0; i0 < D.b_n_ops; i0 += 64) {
        const uint32_t i = i0 + L;
        const bool v = i < D.b_n_ops;
        const uint4 q = v ? reinterpret_cast<const uint4 *>(B.ops)[i] : uint4{0, 0, 0, 0};
        const uint32_t e = v ? hist::entry_of(B, q.x) : 0;
        const uint32_t ps = v ? umax(S.reach[e], B.ent[2 * e]) : 0;
        const bool inc = v && q.x + q.y > ps;
        uint32_t b0 = 0, b1 = 0;
        if (inc && !(q.w & 1u)) hist::piece_bytes(B, D.b_complete != 0, umax(q.x, ps), q.x + q.y, b0, b1);
        nop += popc(ballot(inc));
        ntext += wave_sum(b1 - b0);
    }
    uint32_t nm = 0;
    for (uint32_t a = L; a < D.b_n_agents; a += 64) {
        const uint32_t len = B.agents[2 * a + 1];
        nm += leb_len(len) + len;
    }
    C.n_names = wave_sum(nm);
    C.n_pieces = np; C.n_lv = nlv; C.n_par = npar; C.n_ar = nar; C.n_op = nop; C.n_text = ntext;
}

__global__ __launch_bounds__(64) void patch_mark_kernel(PatchParams P) {
    extern __shared__ uint32_t lds[];
    const uint32_t doc = blockIdx.x;
    if (doc >= P.n_docs) return;
    const HistDesc D = P.H.docs[doc];
    PatchCounts C{};
    hist::Counts R{};
    uint32_t st = D.skip;
    if (!st) st = hist::mark_doc(P.H, D, lds, R);
    if (!st) count_patch(P.H, D, C);
    if (lane() == 0) {
        PatchCounts &o = P.counts[doc];
        o.status = st; o.n_front = st ? 0u : R.n_version;
        o.n_pieces = C.n_pieces; o.n_lv = C.n_lv; o.n_par = C.n_par; o.n_ar = C.n_ar; o.n_op = C.n_op; o.n_text = C.n_text;
        o.n_names = C.n_names; o.form = D.skip ? 0u : D.use_lds ? 1u : 2u;
    }
}

// ---- build -----------------------------------------------------------------------------------
struct Scratch {
    uint32_t *pieceof;                                  // base entry -> piece (NONE: no new ops)
    uint32_t *pstart, *pend, *pent, *fullnp, *pending;  // per piece: LVs, entry, parents in the graph, unvisited in-patch parents
    uint32_t *coff, *ccur, *pa0, *po0;                  // children CSR offsets / cursors, first agent run, first op run
    uint32_t *stack, *order, *outpos;                   // the walk's stack, walk step -> piece, piece -> output LV
    uint32_t *clist;                                    // children
    uint32_t *ppoff, *pinfo;                            // first parent slot of a piece; two words per parent (see D)
    uint32_t *amap, *alast, *ainv;                      // agent -> mapped id (0: none), end of its last seq range; id - 1 -> agent
    uint32_t *oppiece, *oprec;                          // 8 words per op-run piece, 4 per merged op run
    uint8_t *aab, *txb, *verb, *text, *lzb;
};

DEV Scratch scratch_of(const PatchParams &P, const PatchDesc &D, uint32_t ne, uint32_t n_agents) {
    Scratch W;
    uint32_t *w = P.w + D.w_off;
    const uint32_t np = D.n_pieces;
    W.pieceof = w; w += ne;
    W.pstart = w; w += np; W.pend = w; w += np; W.pent = w; w += np; W.fullnp = w; w += np; W.pending = w; w += np;
    W.coff = w; w += np + 1; W.ccur = w; w += np; W.pa0 = w; w += np; W.po0 = w; w += np;
    W.stack = w; w += np; W.order = w; w += np; W.outpos = w; w += np;
    W.clist = w; w += D.n_par;
    W.ppoff = w; w += np; W.pinfo = w; w += 2ull * D.n_par;
    W.amap = w; w += n_agents; W.alast = w; w += n_agents; W.ainv = w; w += n_agents;
    W.oppiece = w; w += 8ull * D.n_op;
    W.oprec = w;
    uint8_t *b = P.b + D.b_off;
    W.aab = b; b += D.c_aa; W.txb = b; b += D.c_tx; W.verb = b; b += PATCH_FRONT_BYTES;
    b += (16 - (reinterpret_cast<uintptr_t>(b) & 15)) & 15;
    W.text = b; b += (D.n_text + 15) & ~15u;
    W.lzb = b;
    return W;
}

// a byte stream written by lane 0 (the sequential record mergers' output), its length wave-uniform
struct Stream {
    uint8_t *p;
    uint32_t n, cap;
    bool over;
};
DEV void sput(Stream &s, uint64_t v) {
    const uint32_t k = leb_len(v);
    if (s.n + k > s.cap) { s.over = true; return; }
    if (lane() == 0) put_leb(s.p + s.n, v);
    s.n += k;
}

__global__ __launch_bounds__(64) void patch_build_kernel(PatchParams P) {
    __shared__ __attribute__((aligned(16))) uint32_t tab[4096];   // LZ4 hash table, then the CRC table
    __shared__ __attribute__((aligned(16))) uint8_t lring[enc::LZ_RING];
    const uint32_t doc = blockIdx.x;
    if (doc >= P.n_docs) return;
    const PatchDesc PD = P.docs[doc];
    const uint32_t L = lane();
    PatchResult R{};
    auto finish = [&](uint32_t st) {
        if (L == 0) {
            PatchResult &o = P.results[doc];
            o.status = st; o.len = st ? 0u : R.len;
            o.n_walk = R.n_walk; o.n_op_runs = R.n_op_runs; o.n_agent_runs = R.n_agent_runs; o.n_txns = R.n_txns;
            o.n_mapped = R.n_mapped; o.text_len = R.text_len; o.lz_len = R.lz_len; o.pad = 0;
            for (int k = 0; k < 7; k++) o.cyc[k] = R.cyc[k];
        }
    };
    if (PD.skip) { finish(PD.skip); return; }
    uint64_t t_prev = P.prof ? clock64() : 0;
    auto mark = [&](int k) {   // phase cycles, when the call asked for them
        if (!P.prof) return;
        const uint64_t t = clock64();
        R.cyc[k] = uint32_t(t - t_prev);
        t_prev = t;
    };
    const HistDesc HD = P.H.docs[doc];
    const Base B = hist::base_of(P.H, HD);
    const Scr S = hist::scr_of(P.H, HD);
    const uint32_t ne = B.ne, np = PD.n_pieces, n_ar = HD.b_n_aruns, n_ops = HD.b_n_ops, n_agents = HD.b_n_agents;
    const Scratch W = scratch_of(P, PD, ne, n_agents);
    const uint4 *aruns = reinterpret_cast<const uint4 *>(B.aruns);
    const uint4 *ops = reinterpret_cast<const uint4 *>(B.ops);
    const bool store_text = P.flags & 1u, compress = P.flags & 2u, complete = HD.b_complete != 0;
    uint8_t *out = P.out + PD.out_off;

    // ---- A: pieces -----------------------------------------------------------------------------
    {
        uint32_t k0 = 0;
        for (uint32_t e0 = 0; e0 < ne; e0 += 64) {
            const uint32_t e = e0 + L;
            const bool valid = e < ne;
            const uint32_t st = valid ? B.ent[2 * e] : 0, en = valid ? B.ent[2 * e + 1] : 0;
            const uint32_t ps = umax(valid ? S.reach[e] : 0, st);
            const bool pc = valid && ps < en;
            const uint64_t m = ballot(pc);
            const uint32_t k = k0 + popc(m & lt_mask());
            const bool fits = pc && k < np;
            if (valid) W.pieceof[e] = fits ? k : NONE;
            if (fits) {
                W.pstart[k] = ps; W.pend[k] = en; W.pent[k] = e;
                W.fullnp[k] = ps > st ? 1u : B.poff[e + 1] - B.poff[e];
                W.pa0[k] = find_le(B.aruns, 4, n_ar, ps);
                W.po0[k] = find_le(B.ops, 4, n_ops, ps);
                W.ccur[k] = 0;
            }
            k0 += popc(m);
        }
        if (k0 != np) { finish(ErrCapacity); return; }
    }
    for (uint32_t i = L; i < n_agents; i += 64) { W.amap[i] = 0; W.alast[i] = 0; }
    fence_agent();

    // ---- B: edges ------------------------------------------------------------------------------
    // in-patch parent of piece k, entry parent slot j: the parent's piece, or NONE
    auto parent_piece = [&](uint32_t p) -> uint32_t {
        const uint32_t pp = ldw(&W.pieceof[hist::entry_of(B, p)]);
        return (pp != NONE && p >= ldw(&W.pstart[pp])) ? pp : NONE;
    };
    for (uint32_t k = L; k < np; k += 64) {   // count
        const uint32_t e = W.pent[k];
        uint32_t mine = 0;
        if (W.pstart[k] == B.ent[2 * e]) {
            for (uint32_t j = B.poff[e]; j < B.poff[e + 1]; j++) {
                const uint32_t pp = parent_piece(B.par[j]);
                if (pp != NONE) { atomicAdd(&W.ccur[pp], 1u); mine++; }
            }
        }
        W.pending[k] = mine;
    }
    fence_agent();
    uint32_t n_edges = 0, n_roots = 0;
    for (uint32_t k0 = 0; k0 < np; k0 += 64) {   // offsets
        const uint32_t k = k0 + L;
        const bool v = k < np;
        const uint32_t c = v ? __hip_atomic_load(&W.ccur[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        const uint32_t incl = scan_incl(c);
        if (v) { W.coff[k] = n_edges + incl - c; W.ccur[k] = 0; }
        n_edges += rdl(incl, 63);
        n_roots += popc(ballot(v && ldw(&W.pending[k]) == 0));
    }
    if (L == 0) W.coff[np] = n_edges;
    if (n_edges > PD.n_par) { finish(ErrCapacity); return; }
    fence_agent();
    for (uint32_t k = L; k < np; k += 64) {   // fill
        const uint32_t e = W.pent[k];
        if (W.pstart[k] == B.ent[2 * e]) {
            for (uint32_t j = B.poff[e]; j < B.poff[e + 1]; j++) {
                const uint32_t pp = parent_piece(B.par[j]);
                if (pp != NONE) {
                    const uint32_t slot = ldw(&W.coff[pp]) + atomicAdd(&W.ccur[pp], 1u);
                    if (slot < n_edges) W.clist[slot] = k;
                }
            }
        }
    }
    fence_agent();
    for (uint32_t k = L; k < np; k += 64) {   // children in ascending piece order
        const uint32_t c0 = ldw(&W.coff[k]), c1 = ldw(&W.coff[k + 1]);
        for (uint32_t i = c0 + 1; i < c1; i++) {
            const uint32_t v = __hip_atomic_load(&W.clist[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            uint32_t j = i;
            for (; j > c0; j--) {
                const uint32_t u = __hip_atomic_load(&W.clist[j - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (u <= v) break;
                W.clist[j] = u;
            }
            W.clist[j] = v;
        }
    }
    {   // the initial stack: the parentless pieces, reversed
        uint32_t r0 = 0;
        for (uint32_t k0 = 0; k0 < np; k0 += 64) {
            const uint32_t k = k0 + L;
            const bool root = k < np && ldw(&W.pending[k]) == 0;
            const uint64_t m = ballot(root);
            const uint32_t r = r0 + popc(m & lt_mask());
            if (root && r < n_roots) W.stack[n_roots - 1 - r] = k;
            r0 += popc(m);
        }
    }
    fence_agent();
    mark(0);

    // ---- C: walk -------------------------------------------------------------------------------
    uint32_t nw = 0;
    for (uint32_t sp = n_roots; sp && nw < np;) {
        const uint32_t top = ldw(&W.stack[sp - 1]);
        uint32_t idx = top;
        if (ldw(&W.fullnp[top]) >= 2) {   // prefer a non-merge (txn_trace.rs:243-265)
            for (int64_t hi = int64_t(sp) - 1; hi > 0; hi -= 64) {   // stack slots [hi - 64, hi), nearest the top first
                const int64_t pos = hi - 1 - int64_t(L);
                const uint32_t cand = pos >= 0 ? ldw(&W.stack[pos]) : 0;
                const bool ok = pos >= 0 && ldw(&W.fullnp[cand]) < 2;
                const uint64_t m = ballot(ok);
                if (m) {
                    const uint32_t b = ctz(m);
                    idx = rdl(cand, b);
                    if (L == b) W.stack[pos] = top;
                    break;
                }
            }
        }
        sp--;
        if (L == 0) W.order[nw] = idx;
        nw++;
        const uint32_t c0 = ldw(&W.coff[idx]), c1 = ldw(&W.coff[idx + 1]);
        for (uint32_t c = c0; c < c1; c += 64) {
            const bool v = c + L < c1;
            const uint32_t ch = v ? ldw(&W.clist[c + L]) : 0;
            const uint32_t left = v ? ldw(&W.pending[ch]) - 1 : 1;
            if (v) W.pending[ch] = left;
            const uint64_t m = ballot(v && left == 0);
            const uint32_t at = sp + popc(m & lt_mask());
            if (v && left == 0 && at < np) W.stack[at] = ch;
            sp += popc(m);
        }
        if (sp > np) break;
        fence_workgroup();
    }
    if (nw != np) { finish(ErrCapacity); return; }   // (unreachable: every piece has a path from a parentless one)
    fence_workgroup();
    {   // every piece's output position: the prefix sum of the piece lengths in walk order
        uint32_t tot = 0;
        for (uint32_t k0 = 0; k0 < nw; k0 += 64) {
            const uint32_t k = k0 + L;
            const uint32_t pc = k < nw ? ldw(&W.order[k]) : 0;
            const uint32_t len = k < nw ? ldw(&W.pend[pc]) - ldw(&W.pstart[pc]) : 0;
            const uint32_t incl = scan_incl(len);
            if (k < nw) W.outpos[pc] = tot + incl - len;
            tot += rdl(incl, 63);
        }
        if (tot != PD.n_lv) { finish(ErrCapacity); return; }
    }
    fence_workgroup();
    R.n_walk = nw;
    mark(1);

    // ---- D: records ------------------------------------------------------------------------------
    uint32_t n_mapped = 0;
    auto map_agent = [&](uint32_t a) -> uint32_t {   // AgentMapping::map (encode_oplog.rs:191-240)
        uint32_t m = ldw(&W.amap[a]);
        if (!m) {
            m = ++n_mapped;
            if (L == 0) { W.amap[a] = m; W.ainv[m - 1] = a; }
            fence_workgroup();
        }
        return m;
    };
    auto agent_version = [&](uint32_t lv, uint32_t &agent, uint32_t &seq) {
        const uint4 A = aruns[find_le(B.aruns, 4, n_ar, lv)];
        agent = A.z;
        seq = A.w + (lv - A.x);
    };
    Stream aa{W.aab, 0, PD.c_aa, false}, tx{W.txb, 0, PD.c_tx, false}, ver{W.verb, 0, PATCH_FRONT_BYTES, false};
    uint32_t naa = 0, ntx = 0;
    bool aa_have = false;   // the open agent assignment run (encode_oplog.rs:142-189)
    uint32_t aaA = 0, aaL = 0;
    int64_t aaD = 0;
    auto aa_flush = [&]() {
        if (!aa_have) return;
        const bool jump = aaD != 0;
        sput(aa, uint64_t(aaA) * 2 + (jump ? 1 : 0));
        sput(aa, aaL);
        if (jump) sput(aa, zz_old(aaD));
        naa++;
    };
    // every parent of every piece, resolved lane-parallel before the record loop: (output LV of the
    // parent, NONE) when it lies inside the patch -- every in-patch parent is walked, hence
    // written, before its child -- else its (agent, seq)
    {
        uint32_t tot = 0;
        bool over = false;
        for (uint32_t k0 = 0; k0 < np; k0 += 64) {
            const uint32_t k = k0 + L;
            const bool v = k < np;
            const uint32_t cnt = v ? ldw(&W.fullnp[k]) : 0, incl = scan_incl(cnt), off = tot + incl - cnt;
            if (v) {
                W.ppoff[k] = off;
                if (off + cnt <= PD.n_par) {
                    const uint32_t s = ldw(&W.pstart[k]), e = ldw(&W.pent[k]), p0 = B.poff[e];
                    const bool inside = s > B.ent[2 * e];
                    for (uint32_t j = 0; j < cnt; j++) {
                        const uint32_t p = inside ? s - 1 : B.par[p0 + j];
                        const uint32_t pp = parent_piece(p);
                        uint32_t w0, w1 = NONE;
                        if (pp != NONE) w0 = ldw(&W.outpos[pp]) + (p - ldw(&W.pstart[pp]));
                        else agent_version(p, w0, w1);
                        W.pinfo[2ull * (off + j)] = w0;
                        W.pinfo[2ull * (off + j) + 1] = w1;
                    }
                } else {
                    over = true;
                }
            }
            tot += rdl(incl, 63);
        }
        if (ballot(over)) { finish(ErrCapacity); return; }
    }
    fence_workgroup();
    bool tx_have = false;   // the open txn (GraphEntrySimple, graph/mod.rs:239-254): LVs, output start, parents
    uint32_t tx_s = 0, tx_e = 0, tx_out0 = 0, tx_cnt = 0, tx_off = 0, tx_w0 = 0, tx_w1 = 0;
    auto tx_write = [&]() {
        sput(tx, tx_e - tx_s);
        if (tx_cnt == 0) sput(tx, 1);   // ROOT: foreign agent 0
        for (uint32_t j = 0; j < tx_cnt; j++) {
            const uint32_t w0 = j ? ldw(&W.pinfo[2ull * (tx_off + j)]) : tx_w0;
            const uint32_t w1 = j ? ldw(&W.pinfo[2ull * (tx_off + j) + 1]) : tx_w1;
            const uint64_t more = j + 1 < tx_cnt ? 1 : 0;
            if (w1 == NONE) {   // local: an output-order distance
                sput(tx, (uint64_t(tx_out0 - w0) * 2 + more) * 2);
            } else {            // foreign: (mapped agent, seq)
                sput(tx, (uint64_t(map_agent(w0)) * 2 + more) * 2 + 1);
                sput(tx, w1);
            }
        }
        ntx++;
    };
    {
        // 64 walk steps per round in the lanes (piece, first agent run, first parent), the merge
        // decisions wave-uniform over readlane: a step loads only for a second agent run, a
        // change of agent or a second parent
        uint32_t outp = 0, cur_agent = NONE, cur_m = 0, cur_last = 0;
        for (uint32_t k0 = 0; k0 < nw; k0 += 64) {
            const uint32_t k = k0 + L;
            const bool v = k < nw;
            const uint32_t g_pc = v ? ldw(&W.order[k]) : 0;
            const uint32_t g_s = v ? ldw(&W.pstart[g_pc]) : 0, g_e = v ? ldw(&W.pend[g_pc]) : 0;
            const uint32_t g_en = v ? ldw(&W.pent[g_pc]) : 0, g_fnp = v ? ldw(&W.fullnp[g_pc]) : 0;
            const uint32_t g_par0 = !v ? 0u : g_s > B.ent[2 * g_en] ? g_s - 1 : g_fnp ? B.par[B.poff[g_en]] : 0u;
            const uint32_t g_a0 = v ? ldw(&W.pa0[g_pc]) : 0;
            const uint4 g_A = v ? aruns[g_a0] : uint4{0, 0, 0, 0};
            const uint32_t g_off = v ? ldw(&W.ppoff[g_pc]) : 0;
            const uint32_t g_w0 = v && g_fnp ? ldw(&W.pinfo[2ull * g_off]) : 0;
            const uint32_t g_w1 = v && g_fnp ? ldw(&W.pinfo[2ull * g_off + 1]) : 0;
            const uint32_t nk = umin(64u, nw - k0);
            for (uint32_t j = 0; j < nk; j++) {
                const uint32_t s = rdl(g_s, j), e = rdl(g_e, j), fnp = rdl(g_fnp, j), par0 = rdl(g_par0, j);
                uint4 A = uint4{rdl(g_A.x, j), rdl(g_A.y, j), rdl(g_A.z, j), rdl(g_A.w, j)};
                for (uint32_t a = rdl(g_a0, j);;) {   // 1. agent assignment (the first run holds LV s)
                    const uint32_t x = umax(A.x, s), y = umin(A.x + A.y, e);
                    if (x < y) {
                        if (A.z != cur_agent) {   // (the current agent's last seq stays in a register)
                            if (cur_agent != NONE && L == 0) W.alast[cur_agent] = cur_last;
                            fence_workgroup();
                            cur_agent = A.z;
                            cur_m = map_agent(A.z);
                            cur_last = ldw(&W.alast[A.z]);
                        }
                        const uint32_t s0 = A.w + (x - A.x);
                        const int64_t d = int64_t(s0) - int64_t(cur_last);
                        cur_last = s0 + (y - x);
                        if (aa_have && aaA == cur_m && d == 0) {
                            aaL += y - x;
                        } else {
                            aa_flush();
                            aa_have = true; aaA = cur_m; aaD = d; aaL = y - x;
                        }
                    }
                    if (A.x + A.y >= e || ++a >= n_ar) break;
                    A = aruns[a];
                }
                // 3. parents (the ops, 2., touch no agent: they are merged below)
                if (tx_have && s == tx_e && fnp == 1 && par0 == tx_e - 1) {
                    tx_e = e;
                } else {
                    if (tx_have) tx_write();
                    tx_have = true; tx_s = s; tx_e = e; tx_out0 = outp;
                    tx_cnt = fnp; tx_off = rdl(g_off, j); tx_w0 = rdl(g_w0, j); tx_w1 = rdl(g_w1, j);
                }
                outp += e - s;
            }
        }
        aa_flush();
        if (tx_have) tx_write();
        const uint32_t *front = P.H.o_front + HD.o_ver;   // the StartBranch version (write_version)
        for (uint32_t i = 0; i < PD.n_front; i++) {
            uint32_t agent, seq;
            agent_version(front[i], agent, seq);
            sput(ver, uint64_t(map_agent(agent)) * 2 + (i + 1 < PD.n_front ? 1 : 0));
            sput(ver, seq);
        }
    }
    if (aa.over || tx.over || ver.over) { finish(ErrCapacity); return; }
    mark(2);

    // op-run pieces in walk order: (start, end, del | fwd << 1, first LV, end LV, content bytes)
    uint32_t nopp = 0;
    {
        bool over = false;
        for (uint32_t k0 = 0; k0 < nw; k0 += 64) {
            const uint32_t k = k0 + L;
            const bool v = k < nw;
            const uint32_t pc = v ? ldw(&W.order[k]) : 0;
            const uint32_t s = v ? ldw(&W.pstart[pc]) : 0, e = v ? ldw(&W.pend[pc]) : 0;
            const uint32_t i0 = v ? ldw(&W.po0[pc]) : 0, i1 = v ? find_le(B.ops, 4, n_ops, e - 1) : 0;
            const uint32_t cnt = v ? i1 - i0 + 1 : 0, incl = scan_incl(cnt), off = nopp + incl - cnt;
            if (v) {
                if (off + cnt <= PD.n_op) {
                    for (uint32_t i = i0; i <= i1; i++) {
                        const uint4 q = ops[i];
                        const uint32_t x = umax(q.x, s), y = umin(q.x + q.y, e), kk = x - q.x, m = y - x;
                        const bool del = q.w & 1u, fwd = (q.w >> 1) & 1u;
                        uint32_t st = q.z, fw = 1;
                        if (!del) st = q.z + kk;
                        else if (!(fwd || q.y == 1)) { st = q.z + (q.y - kk - m); fw = 0; }
                        uint32_t *w = W.oppiece + 8ull * (off + (i - i0));
                        w[0] = st; w[1] = st + m; w[2] = (del ? 1u : 0u) | (fw << 1); w[3] = x; w[4] = y;
                        uint32_t c0 = NONE, c1 = NONE;
                        if (!del) {
                            c0 = B.cbyte[x];
                            const uint32_t lb = B.cbyte[y - 1];
                            if (lb != NONE) c1 = lb + utf8_len(B.content[lb]);
                        }
                        w[5] = c0; w[6] = c1;
                    }
                } else {
                    over = true;
                }
            }
            nopp += rdl(incl, 63);
        }
        if (ballot(over)) { finish(ErrCapacity); return; }
    }
    fence_workgroup();
    // the ListOpMetrics merge (op_metrics.rs:235-293; can_append / append in dt_encode.cpp): 64
    // pieces per step in the lanes, the merge decisions wave-uniform over readlane
    uint32_t nrec = 0, n_ins = 0, text_len = 0;
    bool unknown = false;
    {
        bool have = false;
        uint32_t aS = 0, aE = 0, aK = 0, aF = 0, aHC = 0, aC1 = 0;
        auto flush = [&]() {
            if (nrec < PD.c_oprec && L == 0) {
                uint32_t *w = W.oprec + 4ull * nrec;
                w[0] = aS; w[1] = aE; w[2] = aK | (aF << 1);
            }
            nrec++;
        };
        auto push = [&](uint32_t bS, uint32_t bE, uint32_t K, uint32_t F, uint32_t HC, uint32_t C0, uint32_t C1) {
            if (have) {
                bool ok = aK == K && aHC == HC && (!HC || aC1 == C0);
                if (ok) {
                    const uint32_t al = aE - aS, bl = bE - bS;
                    const bool af = al == 1 || aF, bf = bl == 1 || F, ar = al == 1 || !aF, br = bl == 1 || !F;
                    ok = (af && bf && ((K == 0 && bS == aE) || (K == 1 && bS == aS))) || (K == 1 && ar && br && bE == aS);
                }
                if (ok) {
                    aF = (bS >= aS && (bS != aS || aK == 1)) ? 1u : 0u;
                    if (aK == 1 && !aF) aS = bS; else aE += bE - bS;
                    if (aHC) aC1 = C1;
                    return;
                }
                flush();
            }
            have = true; aS = bS; aE = bE; aK = K; aF = F; aHC = HC; aC1 = C1;
        };
        for (uint32_t c0 = 0; c0 < nopp; c0 += 64) {
            const uint32_t i = c0 + L;
            uint32_t f[7] = {0, 0, 0, 0, 0, 0, 0};
            if (i < nopp) {
                const uint32_t *w = W.oppiece + 8ull * i;
#pragma unroll
                for (int t = 0; t < 7; t++) f[t] = w[t];
            }
            if (i < nopp && !(f[2] & 1u) && f[5] != NONE && f[6] != NONE) text_len += f[6] - f[5];
            const uint32_t nk = umin(64u, nopp - c0);
            for (uint32_t j = 0; j < nk; j++) {
                const uint32_t bS = rdl(f[0], j), bE = rdl(f[1], j), fl = rdl(f[2], j);
                if (fl & 1u) { push(bS, bE, 1, (fl >> 1) & 1u, 0, 0, 0); continue; }
                n_ins += bE - bS;
                const uint32_t X = rdl(f[3], j), Y = rdl(f[4], j);
                if (complete) {
                    const uint32_t C0 = rdl(f[5], j), C1 = rdl(f[6], j);
                    const bool kn = C0 != NONE && C1 != NONE;
                    if (!kn) unknown = true;
                    push(bS, bE, 0, 1, kn ? 1u : 0u, C0, C1);
                    continue;
                }
                for (uint32_t x = X, y; x < Y; x = y) {   // pieces of uniform ContentIsKnown
                    const uint32_t cx = B.cbyte[x];
                    const bool kn = cx != NONE;
                    y = Y;
                    for (uint32_t b = x + 1; b < Y; b += 64) {
                        const bool diff = b + L < Y && (B.cbyte[b + L] != NONE) != kn;
                        const uint64_t m = ballot(diff);
                        if (m) { y = b + ctz(m); break; }
                    }
                    uint32_t C1 = NONE;
                    if (kn) { const uint32_t lb = B.cbyte[y - 1]; C1 = lb + utf8_len(B.content[lb]); }
                    else unknown = true;
                    push(bS + (x - X), bS + (y - X), 0, 1, kn ? 1u : 0u, cx, C1);
                }
            }
        }
        if (have) flush();
        text_len = wave_sum(text_len);
    }
    if (nrec > PD.c_oprec) { finish(ErrCapacity); return; }
    if (store_text && unknown) { finish(ErrCheckout); return; }   // the reference asserts content.is_some()
    if (!store_text) text_len = 0;
    if (text_len > PD.n_text) { finish(ErrCapacity); return; }
    fence_workgroup();
    mark(3);

    // ---- E: sizes, text, LZ4 -------------------------------------------------------------------
    // (an op record's cursor is its predecessor's op_end: write_op, encode_oplog.rs:20-92)
    auto op_bytes_of = [&](uint32_t i, uint64_t &n, int64_t &d, bool &hd) -> uint32_t {
        const uint32_t *w = W.oprec + 4ull * i;
        uint32_t cursor = 0, oe;
        if (i > 0) {
            uint64_t n2; int64_t d2; bool h2;
            enc::op_code(make_uint4(w[-4], w[-3], w[-2], 0), 0, n2, d2, h2, cursor);
        }
        enc::op_code(make_uint4(w[0], w[1], w[2], 0), cursor, n, d, hd, oe);
        return leb_len(n) + (hd ? leb_len(zz_old(d)) : 0);
    };
    uint32_t op_bytes = 0, nm_bytes = 0;
    for (uint32_t i = L; i < nrec; i += 64) {
        uint64_t n; int64_t d; bool hd;
        op_bytes += op_bytes_of(i, n, d, hd);
    }
    const uint2 *names = reinterpret_cast<const uint2 *>(B.agents);
    for (uint32_t i = L; i < n_mapped; i += 64) {
        const uint32_t nl = names[ldw(&W.ainv[i])].y;
        nm_bytes += leb_len(nl) + nl;
    }
    op_bytes = wave_sum(op_bytes);
    nm_bytes = wave_sum(nm_bytes);
    if (text_len) {   // the inserted content in walk order
        uint32_t tpos = 0;
        for (uint32_t i0 = 0; i0 < nopp; i0 += 64) {
            const uint32_t i = i0 + L;
            uint32_t tl = 0, cb = 0;
            if (i < nopp) {
                const uint32_t *w = W.oppiece + 8ull * i;
                if (!(w[2] & 1u)) { cb = w[5]; tl = w[6] - w[5]; }
            }
            const uint32_t incl = scan_incl(tl);
            uint8_t *d = W.text + tpos + incl - tl;
            // a short run's bytes by its own lane, a long one's (a paste) by the whole wave
            const bool fits = tpos + incl <= PD.n_text, big = tl > 32;
            if (fits && !big)
                for (uint32_t x = 0; x < tl; x++) d[x] = B.content[cb + x];
            for (uint64_t m = ballot(fits && big); m; m &= m - 1) {
                const uint32_t b = ctz(m);
                enc::copy_bytes(W.text + tpos + rdl(incl - tl, b), B.content + rdl(cb, b), rdl(tl, b));
            }
            tpos += rdl(incl, 63);
        }
        if (tpos != text_len) { finish(ErrCapacity); return; }
    }
    fence_workgroup();
    mark(4);
    const bool use_lz = compress && text_len >= 20;
    uint32_t lz_len = 0;
    if (use_lz) {
        enc::Lz z;
        z.prof = false;
        z.in = W.text;
        z.out = W.lzb;
        z.ring = lring;
        z.n = text_len;
        z.tab = tab;
        lz_len = z.run();
        fence_workgroup();
    }

    mark(5);
    // ---- layout and write (encode_dt's chunk order) ----------------------------------------------
    const bool has_doc_id = PD.doc_id_len != NONE;
    const uint32_t lz_body = use_lz ? leb_len(text_len) + lz_len : 0;
    const uint32_t lz_chunk = use_lz ? 1 + leb_len(lz_body) + lz_body : 0;
    const uint32_t docid_body = has_doc_id ? 1 + PD.doc_id_len : 0;
    const uint32_t fi_body = (has_doc_id ? 1 + leb_len(docid_body) + docid_body : 0) + 1 + leb_len(nm_bytes) + nm_bytes;
    const uint32_t sb_body = PD.n_front ? 1 + leb_len(ver.n) + ver.n : 0;
    const uint32_t content_body = use_lz ? 1 + leb_len(text_len) : 1 + text_len;
    const uint64_t known_v = uint64_t(n_ins) * 2 + 1;   // every stored insert is known: one run
    const uint32_t known_body = leb_len(known_v);
    const uint32_t pc_body = 1 + (1 + leb_len(content_body) + content_body) + (1 + leb_len(known_body) + known_body);
    const uint32_t pc_chunk = text_len ? 1 + leb_len(pc_body) + pc_body : 0;
    const uint32_t patches_body = pc_chunk + (1 + leb_len(aa.n) + aa.n) + (1 + leb_len(op_bytes) + op_bytes) +
                                  (1 + leb_len(tx.n) + tx.n);
    const uint64_t total64 = 9ull + lz_chunk + (1 + leb_len(fi_body) + fi_body) + (1 + leb_len(sb_body) + sb_body) +
                             (1 + leb_len(patches_body) + uint64_t(patches_body)) + 6;
    if (total64 > PD.out_cap) { finish(ErrCapacity); return; }
    uint32_t at = 0;
    auto hbyte = [&](uint8_t v) { if (L == 0) out[at] = v; at++; };
    auto hleb = [&](uint64_t v) { if (L == 0) put_leb(out + at, v); at += leb_len(v); };
    auto hcopy = [&](const uint8_t *src, uint32_t n) { enc::copy_bytes(out + at, src, n); at += n; };
    {
        const uint8_t magic[8] = {'D', 'M', 'N', 'D', 'T', 'Y', 'P', 'S'};
        for (int i = 0; i < 8; i++) hbyte(magic[i]);
        hbyte(0);   // PROTOCOL_VERSION
    }
    if (use_lz) {
        hbyte(enc::C_LZ4); hleb(lz_body); hleb(text_len);
        hcopy(W.lzb, lz_len);
    }
    hbyte(enc::C_FILEINFO); hleb(fi_body);
    if (has_doc_id) {
        hbyte(enc::C_DOCID); hleb(docid_body); hbyte(4);   // DataType::PlainText
        hcopy(B.in + PD.doc_id_off, PD.doc_id_len);
    }
    hbyte(enc::C_AGENTNAMES); hleb(nm_bytes);
    for (uint32_t i0 = 0; i0 < n_mapped; i0 += 64) {   // names in order of first mention
        const uint32_t i = i0 + L;
        uint32_t nb = 0;
        uint2 nmv = make_uint2(0, 0);
        if (i < n_mapped) { nmv = names[ldw(&W.ainv[i])]; nb = leb_len(nmv.y) + nmv.y; }
        const uint32_t incl = scan_incl(nb);
        if (i < n_mapped) {
            uint8_t *d = out + at + incl - nb;
            const uint32_t h = put_leb(d, nmv.y);
            for (uint32_t x = 0; x < nmv.y; x++) d[h + x] = B.in[nmv.x + x];
        }
        at += rdl(incl, 63);
    }
    hbyte(enc::C_STARTBRANCH); hleb(sb_body);
    if (PD.n_front) {
        hbyte(12); hleb(ver.n);   // Version
        hcopy(W.verb, ver.n);
    }
    hbyte(enc::C_PATCHES); hleb(patches_body);
    if (text_len) {   // ContentChunk::flush (encode_oplog.rs:381-398)
        hbyte(enc::C_PATCHCONTENT); hleb(pc_body);
        hbyte(0);   // Ins
        hbyte(use_lz ? enc::C_CONTENTCOMP : enc::C_CONTENT); hleb(content_body); hbyte(4);
        if (use_lz) hleb(text_len);
        else hcopy(W.text, text_len);
        hbyte(enc::C_CONTENTKNOWN); hleb(known_body); hleb(known_v);
    }
    hbyte(enc::C_OPVERSIONS); hleb(aa.n);
    hcopy(W.aab, aa.n);
    hbyte(enc::C_OPTYPEPOS); hleb(op_bytes);
    for (uint32_t i0 = 0; i0 < nrec; i0 += 64) {
        const uint32_t i = i0 + L;
        uint32_t nb = 0;
        uint64_t n = 0;
        int64_t d = 0;
        bool hd = false;
        if (i < nrec) nb = op_bytes_of(i, n, d, hd);
        const uint32_t incl = scan_incl(nb);
        if (i < nrec) {
            uint8_t *p = out + at + incl - nb;
            const uint32_t k = put_leb(p, n);
            if (hd) put_leb(p + k, zz_old(d));
        }
        at += rdl(incl, 63);
    }
    hbyte(enc::C_OPPARENTS); hleb(tx.n);
    hcopy(W.txb, tx.n);
    if (uint64_t(at) + 6 != total64) { finish(ErrCapacity); return; }
    fence_workgroup();
    // ---- CRC-32C over everything before the CRC chunk (encode_oplog.rs:731-734) ------------------
    for (uint32_t i = L; i < 256; i += 64) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
        tab[i] = c;
    }
    fence_workgroup();
    const uint32_t crc = enc::crc32c_par(out, at, tab, P.x2n);
    if (L == 0) {
        uint8_t *p = out + at;
        p[0] = enc::C_CRC; p[1] = 4;
        p[2] = uint8_t(crc); p[3] = uint8_t(crc >> 8); p[4] = uint8_t(crc >> 16); p[5] = uint8_t(crc >> 24);
    }
    mark(6);
    R.len = at + 6;
    R.n_op_runs = nrec; R.n_agent_runs = naa; R.n_txns = ntx; R.n_mapped = n_mapped; R.text_len = text_len; R.lz_len = lz_len;
    finish(S_OK);
}

}  // namespace patch

int launch_patch_mark(const PatchParams &p, void *stream) {
    if (!p.n_docs) return 0;
    if (p.lds_entries > HIST_LDS_ENTRIES) return 65;
    hipLaunchKernelGGL(patch::patch_mark_kernel, dim3(p.n_docs), dim3(64), size_t(p.lds_entries) * 4,
                       reinterpret_cast<hipStream_t>(stream), p);
    return launch_error() == hipSuccess ? 0 : 66;
}

int launch_patch_build(const PatchParams &p, void *stream) {
    if (!p.n_docs) return 0;
    hipLaunchKernelGGL(patch::patch_build_kernel, dim3(p.n_docs), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), p);
    return launch_error() == hipSuccess ? 0 : 66;
}

}  // namespace dtgpu
