// dt_plan.hip -- device walk planner: the decoded oplog of each document -> the replay command
// stream (INS / DEL / TOG commands + retreat/advance entries) consumed by dt_replay.hip.
//
// One wavefront plans one document, walking the causal graph in the reference's spanning-tree
// order (SpanningTreeWalker, src/listmerge/txn_trace.rs:114-333): a todo stack seeded with the
// root entries; merge entries (>= 2 parents) wait while a non-merge entry is ready
// (txn_trace.rs:249-266); an entry becomes ready when its last parent entry is consumed.
//
// Between two consumed entries the tracker moves from the previous entry's last LV to the next
// entry's parents: retreat (ancestors of the old frontier not in the new one) then advance
// (the converse) -- Graph::diff_rev (src/causalgraph/graph/tools.rs:176-292).  The planner gets
// those sets from version vectors over causal chains: the host partitions the graph entries
// into chains (each entry extends the chain whose tail is one of its parents, dt_host.cpp
// build_plan_input), so the ancestor set of a version is a prefix of every chain,
// { (chain, seq) : seq < vv[chain] }, and a diff is one seq range per chain, copied out of a
// dense per-chain seq -> LV table.  (Diamond-types' agents are not chains in general: a git
// import has one author committing on concurrent branches.)
//
// Three planners, one per kind of document:
//   plan_kernel_1     <= 64 chains.  The order is walk_kernel's, always: it runs first (a 16-lane
//                     group per document) and stores each document's spanning-tree order;
//                     plan_doc_split walks nothing, it turns that order into commands, lane = step.
//   plan_kernel_wide  > 64 chains (host-staged batches only).  plan_doc<K> walks and emits entry
//                     by entry; lane l keeps chains l, l + 64, ... of the current vector
//                     (K = PLAN_MAX_AGENTS / 64 chunks), the vv rows live in HBM scratch.
//   plan_kernel_xf    merge requests over projected histories (xwalk / plan_doc_xf).
// The two that walk keep the todo stack and the pending-parent counts in LDS and share the
// seeding and the push; all three share the move to the tip, the result write and bind_doc.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dt_device.hpp"
#include "dt_wave.hpp"

namespace dtgpu {
namespace pdev {
using namespace wave;

struct P {
    // inputs (decoded oplog)
    const uint32_t *erec, *par, *pent, *pch, *pcnt, *child, *doff, *dense, *tip;
    const Cmd *opc;
    uint32_t ne, A, ntip, n_lv;
    // scratch: vv rows in HBM; todo stack and pending parent counts in LDS (u16)
    uint32_t *base;
    const uint32_t *order; // <= 64 chains: walk_kernel's order (ne words)
    const uint32_t *prow;  // <= 64 chains: each entry's parent version vector (row_stride words)
    uint32_t row_stride;
    uint16_t *todo;      // ready entries (PLAN_TODO_CAP slots)
    uint8_t *pending;    // per entry: unvisited parents | merge flag
    // outputs
    Cmd *cmds;
    uint32_t *tlist;
    const uint32_t *walk;  // <= 64 chains: walk_kernel's {status, steps} for this document
    uint32_t ccap, tcap;
    uint32_t count_only;   // sizing pass: count commands and entries, write nothing
    // wave-uniform state
    uint32_t nc, nt, err;
    uint32_t steps, limit;
    uint32_t n_ret, n_adv;
    uint32_t prof;
};
// DTGPU_PLAN_PROF cycle counters: in LDS, so that the (usually off) profile holds no SGPRs
__shared__ uint64_t g_pc[7];   // six phases, then the last timestamp
DEV void tk(const P &p) {
    if (p.prof && lane() == 0) { for (int i = 0; i < 6; i++) g_pc[i] = 0; g_pc[6] = __builtin_amdgcn_s_memtime(); }
}
#define PT(slot) do { if (p.prof) { const uint64_t t_ = __builtin_amdgcn_s_memtime(); \
    if (lane() == 0) { g_pc[slot] += t_ - g_pc[6]; g_pc[6] = t_; } } } while (0)

DEV void fail(P &p, uint32_t code) {
    if (!p.err) p.err = code;
}
DEV bool charge(P &p) {
    if (++p.steps > p.limit) { fail(p, PLAN_ERR_INTERNAL); return false; }
    return true;
}

// Entry record (EREC_WORDS words) lane by lane; R(rw, k) reads word k.
enum {
    R_START = 0, R_END, R_POFF, R_NP, R_OP0, R_NOP, R_CHAIN, R_SEQ0, R_CH0, R_NCH, R_PAR0,
    R_PENT0, R_PCH0, R_PCNT0, R_PENT1, R_PCH1, R_PCNT1, R_LASTCH, R_FIRSTCH
};
DEV uint32_t load_rec(const P &p, uint32_t e) {
    const uint32_t l = lane();
    return l < EREC_WORDS ? p.erec[erec_word(p.ne, e, l)] : 0;
}
DEV uint32_t R(uint32_t rw, int k) { return U(rdl(rw, uint32_t(k))); }

template <int K> struct VV { uint32_t v[K]; };

template <int K> DEV void vv_zero(VV<K> &x) {
#pragma unroll
    for (int k = 0; k < K; k++) x.v[k] = 0;
}
template <int K> DEV void vv_max(VV<K> &x, const VV<K> &y) {
#pragma unroll
    for (int k = 0; k < K; k++) x.v[k] = max(x.v[k], y.v[k]);
}
template <int K> DEV bool vv_differ(const VV<K> &x, const VV<K> &y) {
    bool d = false;
#pragma unroll
    for (int k = 0; k < K; k++) d |= x.v[k] != y.v[k];
    return __ballot(d) != 0;
}
template <int K> DEV void load_row(const P &p, uint32_t e, VV<K> &row) {
    const uint32_t l = lane();
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint32_t a = l + 64 * k;
        row.v[k] = a < p.A ? p.base[size_t(e) * p.A + a] : 0;
    }
}
template <int K> DEV void store_row(P &p, uint32_t e, const VV<K> &row) {
    const uint32_t l = lane();
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint32_t a = l + 64 * k;
        if (a < p.A) p.base[size_t(e) * p.A + a] = row.v[k];
    }
}

// The frontier moves along entry e (chain c, first seq s0) up to LV `upto`: row[c] becomes
// s0 + the entry's LVs so far.  check: the chain must continue exactly where row[c] stands
// (the chain decomposition guarantees it; a mismatch means a corrupt plan input).
template <int K>
DEV void fold_entry(P &p, uint32_t start, uint32_t end, uint32_t upto, uint32_t c, uint32_t s0, VV<K> &row,
                    bool check) {
    const uint32_t l = lane();
    const uint32_t hi = min(end, upto + 1);
    if (c >= p.A || hi <= start) { fail(p, PLAN_ERR_INTERNAL); return; }
    bool bad = false;
#pragma unroll
    for (int k = 0; k < K; k++) {
        if (c == l + 64 * k) {
            if (check && row.v[k] != s0) bad = true;
            row.v[k] = check ? s0 + (hi - start) : max(row.v[k], s0 + (hi - start));
        }
    }
    if (__ballot(bad)) fail(p, PLAN_NOT_CHAIN);
}

// Version vector of the version {lv} (lv inside entry e): the entry's parent vector plus the
// entry's own LVs up to lv.
template <int K> DEV void vv_at(P &p, uint32_t lv, uint32_t e, VV<K> &row) {
    const uint32_t rw = load_rec(p, e);
    load_row(p, e, row);
    fold_entry<K>(p, R(rw, R_START), R(rw, R_END), lv, R(rw, R_CHAIN), R(rw, R_SEQ0), row, false);
}

// Emit the retreat (from has more) / advance (to has more) entries of a diff: per agent one
// seq range of its dense seq -> (LV | is_del) table.  The ranges of one 64-agent chunk are
// gathered together, 64 entries per load.
template <int K>
DEV void emit_diff(P &p, const VV<K> &from, const VV<K> &to, const VV<K> &dlo, const VV<K> &dhi, bool allow_retreat) {
    const uint32_t l = lane();
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint32_t a = l + 64 * k;
        const bool act = a < p.A && from.v[k] != to.v[k];
        const u64 am = __ballot(act);
        if (!am) continue;
        if (__ballot(act && to.v[k] < from.v[k] && !allow_retreat)) { fail(p, PLAN_ERR_INTERNAL); return; }
        const bool adv = to.v[k] > from.v[k];
        const uint32_t s0 = adv ? from.v[k] : to.v[k];
        const uint32_t n = act ? (adv ? to.v[k] - from.v[k] : from.v[k] - to.v[k]) : 0;
        const uint32_t d0 = dlo.v[k], d1 = dhi.v[k];
        if (__ballot(act && d0 + s0 + n > d1)) { fail(p, PLAN_ERR_INTERNAL); return; }
        const uint32_t inc = scan_incl(n);
        const uint32_t total = rdl(inc, 63);
        const uint32_t n_adv = rdl(scan_incl(adv ? n : 0), 63);
        if (uint64_t(p.nt) + total > p.tcap) { fail(p, PLAN_TLIST_FULL); return; }
        if (!p.count_only) {
            const uint32_t src = d0 + s0, off = inc - n;   // per agent lane
            bool bad = false;
            for (uint32_t c = 0; c < total; c += 64) {
                const uint32_t u = c + l;
                uint32_t from_idx = 0, flag = 0;
                for (u64 m = am; m; m &= m - 1) {   // the agent whose output slice holds u
                    const uint32_t j = ctz(m);
                    const uint32_t o = U(rdl(off, j)), nn = U(rdl(n, j));
                    const uint32_t sj = U(rdl(src, j)), fj = U(rdl(adv ? TL_ADV : 0u, j));
                    if (u >= o && u < o + nn) { from_idx = sj + (u - o); flag = fj; }
                }
                if (u < total) {
                    const uint32_t v = p.dense[from_idx];
                    if (v == 0xFFFFFFFFu) bad = true;
                    p.tlist[p.nt + u] = v | flag;
                }
            }
            if (__ballot(bad)) { fail(p, PLAN_ERR_INTERNAL); return; }
        }
        p.nt += total;
        p.n_adv += n_adv;
        p.n_ret += total - n_adv;
    }
}

DEV void push_cmd(P &p, uint32_t op, uint32_t a, uint32_t n, uint32_t pos) {
    if (uint64_t(p.nc) >= p.ccap) { fail(p, PLAN_CMDS_FULL); return; }
    if (lane() == 0 && !p.count_only) p.cmds[p.nc] = Cmd{op, a, n, pos};
    p.nc++;
}

constexpr uint8_t MERGE_BIT = 0x80;   // pending byte: parent count (<= 127) | merge flag

// Next entry to consume: the todo top, unless it is a merge and a non-merge is ready
// (txn_trace.rs:249-266).  Pops it.
DEV uint32_t pick(P &p, uint32_t &top) {
    const uint32_t l = lane();
    uint32_t idx = U(p.todo[top - 1]);
    if (p.pending[idx] & MERGE_BIT) {
        int found = -1;
        for (int hi = int(top) - 1; hi >= 0 && found < 0; hi -= 64) {
            const int i = hi - int(l);
            const bool ok = i >= 0 && !(p.pending[p.todo[i]] & MERGE_BIT);
            const u64 m = __ballot(ok);
            if (m) found = hi - int(ctz(m));
        }
        if (found >= 0) {
            idx = U(p.todo[found]);
            if (l == 0) p.todo[found] = p.todo[top - 1];
            fence_wave();
        }
    }
    top--;
    return idx;
}

// Push the entries e of the `ready` lanes onto the todo stack, in lane order.
DEV bool push_ready(P &p, uint32_t &top, bool ready, uint32_t e) {
    const u64 m = __ballot(ready);
    const uint32_t rank = uint32_t(__popcll(m & ((1ull << lane()) - 1ull)));
    if (top + uint32_t(__popcll(m)) > PLAN_TODO_CAP) { fail(p, PLAN_TODO_FULL); return false; }
    if (ready) p.todo[top + rank] = uint16_t(e);
    top += uint32_t(__popcll(m));
    return true;
}
DEV uint8_t pend_byte(uint32_t np, bool merge) { return uint8_t(min(np, 0x7Fu) | (merge ? MERGE_BIT : 0)); }
// Seed the todo stack from the pending bytes: the roots (no parent left to wait for), highest
// index first, so that the first root ends on top.
DEV void seed_roots(P &p, uint32_t &top) {
    fence_wave();
    for (int c = int((p.ne + 63) / 64) - 1; c >= 0; c--) {
        if (!charge(p)) break;
        const uint32_t e = uint32_t(c) * 64 + (63 - lane());   // descending entry index across lanes
        if (!push_ready(p, top, e < p.ne && (p.pending[e] & 0x7F) == 0, e)) break;
    }
    fence_wave();
}
// The whole-document seeding: every entry's pending byte from its parent count, then the roots.
DEV void seed_doc(P &p, uint32_t &top) {
    bool bad_np = false;
    for (uint32_t e = lane(); e < p.ne; e += 64) {
        const uint32_t np = p.erec[size_t(e) * EREC_HEAD + R_NP];
        bad_np |= np > 0x7Fu;
        p.pending[e] = pend_byte(np, np >= 2);
    }
    seed_roots(p, top);
    if (__ballot(bad_np)) fail(p, PLAN_WIDE_MERGE);
}

// Move the tracker from one version to another: the retreat / advance entries and their TOG.
template <int K>
DEV void move_to(P &p, const VV<K> &from, const VV<K> &to, const VV<K> &dlo, const VV<K> &dhi, bool allow_retreat) {
    if (!vv_differ(from, to)) return;
    const uint32_t t0 = p.nt;
    emit_diff<K>(p, from, to, dlo, dhi, allow_retreat);
    if (!p.err && p.nt > t0) push_cmd(p, CMD_TOG, t0, p.nt - t0, 0);
}
// The last move, to the tip vt (cg.version; the replay then holds the checkout): what it advances
// is the result's n_tip and no part of n_advance.
template <int K>
DEV void move_to_tip(P &p, PlanResult *res, const VV<K> &vf, const VV<K> &vt, const VV<K> &dlo, const VV<K> &dhi,
                     bool allow_retreat) {
    if (p.err || !vv_differ(vf, vt)) return;
    const uint32_t adv0 = p.n_adv;
    move_to<K>(p, vf, vt, dlo, dhi, allow_retreat);
    res->n_tip = uint32_t(p.n_adv - adv0);
    p.n_adv = adv0;
}
DEV void write_result(const P &p, PlanResult *res) {
    if (lane() != 0) return;
    for (int i = 0; i < 6; i++) res->prof[i] = p.prof ? g_pc[i] : 0;
    res->status = p.err;
    res->ncmd = p.nc; res->ntlist = p.nt;
    res->n_retreat = p.n_ret; res->n_advance = p.n_adv;
}

// The planner's view of document pd: its slices of the batch's arrays, the wave's LDS (the todo
// stack, then the pending bytes), empty outputs.  The callers add their scratch (base, order, walk).
DEV void bind_doc(P &p, const PlanParams &Q, const PlanDesc &pd, uint16_t *lds16, uint64_t limit) {
    p.erec = Q.erec + pd.erec_off;
    p.par = Q.par + pd.par_off; p.pent = Q.pent + pd.par_off;
    p.pch = Q.pch + pd.par_off; p.pcnt = Q.pcnt + pd.par_off;
    p.child = Q.child + pd.child_off;
    p.opc = Q.opc + pd.op_off;
    p.doff = Q.doff + pd.doff_off; p.dense = Q.dense + pd.dense_off;
    p.tip = Q.tip + pd.tip_off * 2;
    p.ne = U(pd.ne); p.A = U(pd.n_agents); p.ntip = U(pd.ntip); p.n_lv = U(pd.n_lv);
    p.todo = lds16;
    p.pending = reinterpret_cast<uint8_t *>(lds16 + PLAN_TODO_CAP);
    p.base = nullptr; p.order = nullptr; p.walk = nullptr;
    p.prow = Q.prow + pd.prow_off; p.row_stride = pd.row_stride;
    p.cmds = Q.cmds + pd.cmd_off; p.tlist = Q.tlist + pd.tlist_off;
    p.count_only = Q.count_only;
    p.ccap = Q.count_only ? 0xFFFFFFFFu : U(pd.ccap);
    p.tcap = Q.count_only ? 0xFFFFFFFFu : U(pd.tcap);
    p.nc = p.nt = p.err = 0;
    p.n_ret = p.n_adv = 0;
    p.steps = 0; p.limit = uint32_t(min<uint64_t>(limit, 0xFFFFFFF0ull));
    p.prof = Q.prof;
}

// > 64 chains: walk and emit entry by entry.  Per consumed entry the wave issues one record load
// (as soon as the entry is picked, overlapping the previous entry's emission), one batch of
// independent loads (its op runs and children) and, when the frontier moves sideways, one gather
// per 64 retreat/advance entries.
template <int K>
DEV void plan_doc(P &p, PlanResult *res) {
    const uint32_t l = lane();
    VV<K> vf, vp, dlo, dhi;
    vv_zero(vf);
    // each chain's dense-table slice, kept in registers
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint32_t a = l + 64 * k;
        dlo.v[k] = a < p.A ? p.doff[a] : 0;
        dhi.v[k] = a < p.A ? p.doff[a + 1] : 0;
    }
    uint32_t top = 0;
    seed_doc(p, top);
    tk(p);
    PT(5);
    uint32_t f = 0xFFFFFFFFu;   // current frontier: ROOT or one LV
    bool have = top > 0;
    uint32_t idx = have ? pick(p, top) : 0;
    uint32_t rw = have ? load_rec(p, idx) : 0;
    while (have && !p.err) {
        if (!charge(p)) break;
        // the entry's op runs, agent runs and children: independent loads, issued together
        const uint32_t np = R(rw, R_NP), op0 = R(rw, R_OP0), nop = R(rw, R_NOP), ch0 = R(rw, R_CH0),
                       nch = R(rw, R_NCH), chain = R(rw, R_CHAIN), seq0 = R(rw, R_SEQ0);
        PT(0);
        const uint32_t e_start = R(rw, R_START), e_end = R(rw, R_END);
        // speculation: the entry's last child is usually the next one consumed
        const uint32_t spec = R(rw, R_LASTCH);
        const uint32_t rw_spec = spec != 0xFFFFFFFFu ? load_rec(p, spec) : 0;
        // (four scalars, not a Cmd: a struct assigned under a branch goes through scratch)
        const uint32_t *opw = reinterpret_cast<const uint32_t *>(p.opc);
        uint32_t oc0 = 0, oc1 = 0, oc2 = 0, oc3 = 0;
        if (l < nop && !p.count_only) {
            const size_t w = 4 * size_t(op0 + l);
            oc0 = opw[w]; oc1 = opw[w + 1]; oc2 = opw[w + 2]; oc3 = opw[w + 3];
        }
        const uint32_t ch = l < nch ? p.child[ch0 + l] : 0;
        // version vector of the parents
        if (np == 1 && R(rw, R_PAR0) == f) {
            vp = vf;
        } else {
            // parents' vectors: each parent entry's row plus its chain's ops up to the parent;
            // up to 4 parents' rows in flight at once
            vv_zero(vp);
            const uint32_t po = R(rw, R_POFF);
            for (uint32_t j0 = 0; j0 < np; j0 += 4) {
                uint32_t pe[4], pc[4], pn[4];
                VV<K> t[4];
#pragma unroll
                for (int jj = 0; jj < 4; jj++) {
                    const uint32_t j = j0 + jj;
                    pe[jj] = pc[jj] = pn[jj] = 0;
                    if (j < np) {
                        if (j < 2) {
                            pe[jj] = R(rw, R_PENT0 + 3 * int(j));
                            pc[jj] = R(rw, R_PCH0 + 3 * int(j));
                            pn[jj] = R(rw, R_PCNT0 + 3 * int(j));
                        } else {
                            pe[jj] = U(p.pent[po + j]);
                            pc[jj] = U(p.pch[po + j]);
                            pn[jj] = U(p.pcnt[po + j]);
                        }
                        load_row(p, pe[jj], t[jj]);
                    }
                }
#pragma unroll
                for (int jj = 0; jj < 4; jj++) {
                    if (j0 + jj >= np) break;
                    vv_max(vp, t[jj]);
#pragma unroll
                    for (int k = 0; k < K; k++)
                        if (pc[jj] == l + 64 * uint32_t(k)) vp.v[k] = max(vp.v[k], pn[jj]);
                }
            }
        }
        store_row(p, idx, vp);
        PT(1);
        const VV<K> v_old = vf;
        // the frontier moves to the entry's last LV; its runs must continue the agents' chains
        vf = vp;
        fold_entry<K>(p, e_start, e_end, e_end - 1, chain, seq0, vf, true);
        if (p.err) break;
        // children whose last parent this was become ready (pushed in child index order); the
        // next entry is picked and its record requested before this entry's output is written
        for (uint32_t c = 0; c < nch; c += 64) {
            const uint32_t chv = c == 0 ? ch : (c + l < nch ? p.child[ch0 + c + l] : 0);
            bool ready = false;
            if (c + l < nch) {
                const uint8_t pd = uint8_t(p.pending[chv] - 1);
                p.pending[chv] = pd;
                ready = (pd & 0x7F) == 0;
            }
            if (!push_ready(p, top, ready, chv)) break;
        }
        fence_wave();
        have = top > 0;
        if (have) {
            idx = pick(p, top);
            rw = idx == spec ? rw_spec : load_rec(p, idx);
        }
        PT(2);
        // retreat / advance to the parents, then apply the entry's op runs
        move_to<K>(p, v_old, vp, dlo, dhi, true);
        if (p.err) break;
        PT(3);
        if (uint64_t(p.nc) + nop > p.ccap) { fail(p, PLAN_CMDS_FULL); break; }
        if (!p.count_only) {
            if (l < nop) {
                uint32_t *cw = reinterpret_cast<uint32_t *>(p.cmds) + 4 * size_t(p.nc + l);
                cw[0] = oc0; cw[1] = oc1; cw[2] = oc2; cw[3] = oc3;
            }
            for (uint32_t j = 64 + l; j < nop; j += 64) p.cmds[p.nc + j] = p.opc[op0 + j];
        }
        p.nc += nop;
        f = e_end - 1;
        PT(4);
    }
    if (!p.err) {
        VV<K> vt;
        vv_zero(vt);
        for (uint32_t j = 0; j < p.ntip; j++) {
            VV<K> t;
            vv_at<K>(p, U(p.tip[2 * j]), U(p.tip[2 * j + 1]), t);
            vv_max(vt, t);
        }
        move_to_tip<K>(p, res, vf, vt, dlo, dhi, false);
    }
    write_result(p, res);
}

// ---- <= 64 chains, two phases -----------------------------------------------------------------
//
// The walk order depends only on the graph (children, merge flags), and what a walk step emits
// depends only on the step's entry and the one before it: the frontier before step i is the
// previous entry's parent vector with that entry's own LVs folded in (fold_entry), the frontier it
// moves to is entry i's parent vector.  So:
//   phase A (walk_kernel, launched before this kernel): the spanning-tree order alone -- pick,
//     children bookkeeping, one record load per step -- stored in p.order, its status and step
//     count in p.walk;
//   phase B (here; lane-parallel, lane = walk step): each step's retreat / advance ranges and op
//     runs sized, offsets by prefix sums, then every step's TOG command, tlist slice and op-run
//     commands written by its own lane.
// The order is walk_kernel's and nobody else's: this function walks nothing.  Its output is the
// sequential walk's (plan_doc's, and the host planner's, which the tests compare it with).
constexpr uint32_t kSplitLaneTl = 24, kSplitLaneOps = 8;   // per-lane step writes up to these sizes
constexpr uint32_t kSplitRegChains = 4;   // up to this many moving chains per step: output-parallel chunk writes
constexpr uint32_t kSplitSegChunk = 4096; // ... for chunks writing up to this many entries / commands
constexpr uint32_t kSplitCopyDepth = 8;   // big steps: 8 x 64 dense-table loads per round trip

// The record and the entry's parent version vector (lane = chain), lane by lane.
struct Rec { uint32_t w, row; };
DEV Rec srec(const P &p, uint32_t e) {
    const uint32_t l = lane();
    return Rec{load_rec(p, e), l < p.A ? p.prow[size_t(e) * p.row_stride + l] : 0u};
}
DEV uint32_t F(const Rec &r, int k) { return R(r.w, k); }

DEV void plan_doc_split(P &p, PlanResult *res) {
    const uint32_t l = lane();
    tk(p);
    PT(5);
    // ---- phase A: walk_kernel's order, its status and its step count ----
    const uint32_t *order = p.order;   // ne words
    const uint32_t ns = U(p.walk[1]);
    if (const uint32_t wst = U(p.walk[0]) & 0xFFFFu) fail(p, wst);   // (high 16 bits: the walk's stack depth)
    PT(0);
    // each chain's dense-table slice, in LDS (the todo stack's space: nothing walks here): A + 1
    // offsets, one more than the lanes at 64 chains
    uint32_t *sdoff = reinterpret_cast<uint32_t *>(p.todo);
    for (uint32_t a = l; a <= p.A; a += 64) sdoff[a] = p.doff[a];
    fence_wave();
    // ---- phase B: per step, lane = step ----
    const uint32_t A = p.A, rs = p.row_stride;
    uint32_t err_code = 0, last_e = 0;
    for (uint32_t c0 = 0; c0 < ns && !p.err; c0 += 64) {
        const uint32_t i = c0 + l;
        const bool valid = i < ns;
        const uint32_t e = valid ? order[i] : 0;
        const bool hp = valid && i > 0;
        const uint32_t ep = hp ? order[i - 1] : 0;
        const uint4 *r4 = reinterpret_cast<const uint4 *>(p.erec);   // the heads (32 bytes each)
        const uint4 a0 = r4[size_t(e) * (EREC_HEAD / 4)], a1 = r4[size_t(e) * (EREC_HEAD / 4) + 1];
        uint4 b0 = make_uint4(0, 0, 0, 0), b1 = make_uint4(0, 0, 0, 0);
        if (hp) { b0 = r4[size_t(ep) * (EREC_HEAD / 4)]; b1 = r4[size_t(ep) * (EREC_HEAD / 4) + 1]; }
        const uint32_t e_start = a0.x, e_end = a0.y, op0 = a1.x, nop = a1.y, chain = a1.z, seq0 = a1.w;
        const uint32_t p_start = b0.x, p_end = b0.y, p_chain = b1.z, p_seq0 = b1.w;
        uint32_t code = 0;
        if (valid && (chain >= A || e_end <= e_start)) code = PLAN_ERR_INTERNAL;
        if (valid && p.prow[size_t(e) * rs + min(chain, rs - 1)] != seq0 && !code) code = PLAN_NOT_CHAIN;
        // the frontier before the step (the previous entry folded) against the step's parents
        uint32_t total = 0, nadv = 0;
        // the step's first kSplitRegChains moving chains (ascending): range length, dense source,
        // advance bit; more moving chains than that send the chunk to the per-step writes
        uint32_t sn[kSplitRegChains], ss[kSplitRegChains], sadv = 0, nmov = 0;
#pragma unroll
        for (uint32_t a = 0; a < kSplitRegChains; a++) sn[a] = ss[a] = 0;
        auto chain_diff = [&](uint32_t a, uint32_t to, uint32_t from) {
            if (hp && a == p_chain) from = p_seq0 + (p_end - p_start);
            const bool adv = to > from;
            const uint32_t n = adv ? to - from : from - to;
            const uint32_t s0 = adv ? from : to;
            if (n && sdoff[a] + s0 + n > sdoff[a + 1] && !code) code = PLAN_ERR_INTERNAL;
            total += n;
            nadv += adv ? n : 0;
            if (n) {
#pragma unroll
                for (uint32_t q = 0; q < kSplitRegChains; q++)
                    if (nmov == q) { sn[q] = n; ss[q] = sdoff[a] + s0; }
                if (adv && nmov < kSplitRegChains) sadv |= 1u << nmov;
                nmov++;
            }
        };
        if ((rs & 3u) == 0) {   // rows 16-byte aligned (device staging): four chains per load
            const uint4 *r4e = reinterpret_cast<const uint4 *>(p.prow + size_t(e) * rs);
            const uint4 *r4p = reinterpret_cast<const uint4 *>(p.prow + size_t(ep) * rs);
            for (uint32_t a = 0; a < A; a += 4) {
                const uint4 t4 = valid ? r4e[a / 4] : make_uint4(0, 0, 0, 0);
                const uint4 f4 = hp ? r4p[a / 4] : make_uint4(0, 0, 0, 0);
                chain_diff(a, t4.x, f4.x);
                if (a + 1 < A) chain_diff(a + 1, t4.y, f4.y);
                if (a + 2 < A) chain_diff(a + 2, t4.z, f4.z);
                if (a + 3 < A) chain_diff(a + 3, t4.w, f4.w);
            }
        } else {
            for (uint32_t a = 0; a < A; a++)
                chain_diff(a, valid ? p.prow[size_t(e) * rs + a] : 0u, hp ? p.prow[size_t(ep) * rs + a] : 0u);
        }
        if (!valid) total = nadv = 0;
        const uint32_t ncmd = valid ? (total ? 1u : 0u) + nop : 0u;
        // offsets: prefix sums over the chunk's steps
        const uint32_t ic = scan_incl(ncmd), it = scan_incl(total);
        const uint32_t co = p.nc + ic - ncmd, to0 = p.nt + it - total;
        const uint32_t sum_c = rdl(ic, 63), sum_t = rdl(it, 63);
        const uint32_t sum_adv = rdl(scan_incl(nadv), 63);
        PT(1);
        const u64 em = __ballot(code != 0);
        if (em) {   // the first failing step ends the walk, as a sequential walk stops there
            fail(p, rdl(code, ctz(em)));
            break;
        }
        if (uint64_t(p.nc) + sum_c > p.ccap) { fail(p, PLAN_CMDS_FULL); break; }
        if (uint64_t(p.nt) + sum_t > p.tcap) { fail(p, PLAN_TLIST_FULL); break; }
        // small steps: each lane writes its own step; a step with a long diff or many op runs
        // is written by the whole wave afterwards (a lane copying node_nodecc's thousands of
        // entries alone would serialise the chunk)
        // A <= 4: output-parallel chunk writes, unless the chunk's output is long (node_nodecc's
        // steps retreat / advance thousands of entries each): then step by step, each step's
        // ranges copied contiguously by the whole wave
        const bool seg_chunk = sum_t > kSplitSegChunk || sum_c > kSplitSegChunk;
        const bool outpar = !__ballot(valid && nmov > kSplitRegChains) && !seg_chunk;
        const bool big = valid && (!outpar ? (seg_chunk || total > kSplitLaneTl || nop > kSplitLaneOps) : false);
        if (!p.count_only && outpar) {
            // output-parallel: output u of the chunk belongs to the first step whose inclusive
            // prefix exceeds it (a binary search over the lanes), inside it to the chain range
            // that covers it; 4 x 64 outputs per round, their loads in flight together
            const uint32_t T0 = p.nt, C0 = p.nc;
            bool bad = false;
            for (uint32_t r = 0; r < sum_t; r += 256) {
                uint32_t val[4], fl[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const uint32_t u = r + 64 * uint32_t(q) + l;
                    uint32_t j = 0;
#pragma unroll
                    for (uint32_t st = 32; st; st >>= 1)
                        if (u >= uint32_t(__shfl(int(it), int(j + st - 1)))) j += st;
                    j = min(j, 63u);
                    const uint32_t w = u - (uint32_t(__shfl(int(it), int(j))) - uint32_t(__shfl(int(total), int(j))));
                    const uint32_t av = uint32_t(__shfl(int(sadv), int(j)));
                    uint32_t before = 0, src = 0, f = 0;
                    bool found = false;
#pragma unroll
                    for (uint32_t a = 0; a < kSplitRegChains; a++) {
                        const uint32_t na = uint32_t(__shfl(int(sn[a]), int(j)));
                        const uint32_t sa = uint32_t(__shfl(int(ss[a]), int(j)));
                        if (!found && w < before + na) { src = sa + (w - before); f = (av >> a) & 1u ? TL_ADV : 0u; found = true; }
                        before += na;
                    }
                    val[q] = u < sum_t ? p.dense[src] : 0u;
                    fl[q] = f;
                }
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const uint32_t u = r + 64 * uint32_t(q) + l;
                    if (u < sum_t) {
                        bad |= val[q] == 0xFFFFFFFFu;
                        p.tlist[T0 + u] = val[q] | fl[q];
                    }
                }
            }
            for (uint32_t r = 0; r < sum_c; r += 256) {   // 4 x 64 commands per round
                Cmd cv[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const uint32_t u = r + 64 * uint32_t(q) + l;
                    uint32_t j = 0;
#pragma unroll
                    for (uint32_t st = 32; st; st >>= 1)
                        if (u >= uint32_t(__shfl(int(ic), int(j + st - 1)))) j += st;
                    j = min(j, 63u);
                    const uint32_t k = u - (uint32_t(__shfl(int(ic), int(j))) - uint32_t(__shfl(int(ncmd), int(j))));
                    const uint32_t tj = uint32_t(__shfl(int(total), int(j))), t0j = uint32_t(__shfl(int(to0), int(j)));
                    const uint32_t o0j = uint32_t(__shfl(int(op0), int(j)));
                    cv[q] = Cmd{CMD_TOG, t0j, tj, 0};
                    if (u < sum_c && !(tj && k == 0)) cv[q] = p.opc[o0j + k - (tj ? 1u : 0u)];
                }
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const uint32_t u = r + 64 * uint32_t(q) + l;
                    if (u < sum_c) p.cmds[C0 + u] = cv[q];
                }
            }
            if (bad) err_code = PLAN_ERR_INTERNAL;
        }
        if (!p.count_only && valid && !big && !outpar) {
            uint32_t cw = co;
            bool bad = false;
            if (total) {
                p.cmds[cw++] = Cmd{CMD_TOG, to0, total, 0};
                uint32_t u = to0;
                for (uint32_t a = 0; a < A; a++) {
                    const uint32_t to = p.prow[size_t(e) * rs + a];
                    uint32_t from = hp ? p.prow[size_t(ep) * rs + a] : 0;
                    if (hp && a == p_chain) from = p_seq0 + (p_end - p_start);
                    if (to == from) continue;
                    const bool adv = to > from;
                    const uint32_t n = adv ? to - from : from - to;
                    const uint32_t src = sdoff[a] + (adv ? from : to), fl = adv ? TL_ADV : 0u;
                    uint32_t k = 0;
                    for (; k + 4 <= n; k += 4) {   // four loads in flight per round
                        uint32_t v[4];
#pragma unroll
                        for (int q = 0; q < 4; q++) v[q] = p.dense[src + k + q];
#pragma unroll
                        for (int q = 0; q < 4; q++) { bad |= v[q] == 0xFFFFFFFFu; p.tlist[u + q] = v[q] | fl; }
                        u += 4;
                    }
                    for (; k < n; k++) {
                        const uint32_t v = p.dense[src + k];
                        bad |= v == 0xFFFFFFFFu;
                        p.tlist[u++] = v | fl;
                    }
                }
            }
            for (uint32_t j = 0; j < nop; j++) p.cmds[cw + j] = p.opc[op0 + j];
            if (bad) err_code = PLAN_ERR_INTERNAL;
        }
        PT(2);
        if (!p.count_only) {
            for (u64 bm = __ballot(big); bm; bm &= bm - 1) {   // the big steps, one at a time
                const uint32_t j = ctz(bm);
                const uint32_t be = U(rdl(e, j)), bep = U(rdl(ep, j)), bhp = U(rdl(hp ? 1u : 0u, j));
                const uint32_t bpc = U(rdl(p_chain, j)), bpv = U(rdl(p_seq0 + (p_end - p_start), j));
                const uint32_t bto = U(rdl(to0, j)), bco = U(rdl(co, j)), btot = U(rdl(total, j));
                const uint32_t bop0 = U(rdl(op0, j)), bnop = U(rdl(nop, j));
                uint32_t cw = bco;
                if (btot) {
                    if (l == 0) p.cmds[cw] = Cmd{CMD_TOG, bto, btot, 0};
                    cw++;
                    // lane = chain: its range, its offset in the step's slice, then 64 outputs per round
                    const uint32_t to = l < A ? p.prow[size_t(be) * rs + l] : 0u;
                    uint32_t from = bhp && l < A ? p.prow[size_t(bep) * rs + l] : 0u;
                    if (bhp && l == bpc) from = bpv;
                    const bool adv = to > from;
                    const uint32_t n = adv ? to - from : from - to;
                    const uint32_t src = (l < A ? sdoff[l] : 0u) + (adv ? from : to), fl = adv ? TL_ADV : 0u;
                    const uint32_t off = scan_incl(n) - n;
                    bool bad = false;
                    for (u64 am = __ballot(n != 0); am; am &= am - 1) {
                        const uint32_t a = ctz(am);
                        const uint32_t o = U(rdl(off, a)), nn = U(rdl(n, a)), sa = U(rdl(src, a)), fa = U(rdl(fl, a));
                        for (uint32_t u0 = 0; u0 < nn; u0 += 64 * kSplitCopyDepth) {   // loads in flight together
                            uint32_t v[kSplitCopyDepth];
#pragma unroll
                            for (int q = 0; q < int(kSplitCopyDepth); q++) {
                                const uint32_t u = u0 + 64 * uint32_t(q) + l;
                                v[q] = u < nn ? p.dense[sa + u] : 0u;
                            }
#pragma unroll
                            for (int q = 0; q < int(kSplitCopyDepth); q++) {
                                const uint32_t u = u0 + 64 * uint32_t(q) + l;
                                if (u < nn) {
                                    bad |= v[q] == 0xFFFFFFFFu;
                                    p.tlist[bto + o + u] = v[q] | fa;
                                }
                            }
                        }
                    }
                    if (__ballot(bad)) err_code = PLAN_ERR_INTERNAL;
                }
                for (uint32_t k = l; k < bnop; k += 64) p.cmds[cw + k] = p.opc[bop0 + k];
            }
        }
        PT(4);
        if (__ballot(err_code != 0)) { fail(p, PLAN_ERR_INTERNAL); break; }
        p.nc += sum_c;
        p.nt += sum_t;
        p.n_adv += sum_adv;
        p.n_ret += sum_t - sum_adv;
        last_e = U(rdl(e, min(63u, ns - 1 - c0)));
    }
    PT(3);
    // the move to the tip starts from the last step's entry folded
    if (!p.err) {
        VV<1> vf;
        vf.v[0] = 0;
        if (ns) {
            const uint32_t rl = load_rec(p, last_e);
            vf.v[0] = l < A ? p.prow[size_t(last_e) * rs + l] : 0u;
            fold_entry<1>(p, R(rl, R_START), R(rl, R_END), R(rl, R_END) - 1, R(rl, R_CHAIN), R(rl, R_SEQ0), vf, false);
        }
        VV<1> dl, dh;
        dl.v[0] = l < A ? sdoff[l] : 0u;
        dh.v[0] = l < A ? sdoff[l + 1] : 0u;
        VV<1> vt;
        vv_zero(vt);
        for (uint32_t j = 0; j < p.ntip && !p.err; j++) {
            const uint32_t tlv = U(p.tip[2 * j]), te = U(p.tip[2 * j + 1]);
            const Rec tr = srec(p, te);
            VV<1> t;
            t.v[0] = tr.row;
            fold_entry<1>(p, F(tr, R_START), F(tr, R_END), tlv, F(tr, R_CHAIN), F(tr, R_SEQ0), t, false);
            vv_max(vt, t);
        }
        move_to_tip<1>(p, res, vf, vt, dl, dh, false);
    }
    write_result(p, res);
}

// K = agent chunks per lane.  Documents with <= 64 agents run in the K = 1 instantiation, the
// others (<= PLAN_MAX_AGENTS) in the wide one; each kernel skips the other's documents.
template <int K>
DEV void plan_entry(const PlanParams &Q) {
    extern __shared__ __attribute__((aligned(16))) uint16_t lds16[];
    if (blockIdx.x >= Q.n_docs) return;
    const uint32_t d = U(Q.doc_list ? Q.doc_list[blockIdx.x] : blockIdx.x);
    const PlanDesc pd = Q.docs[d];
    PlanResult *res = Q.results + d;
    if (pd.skip) return;   // planned on the host
    if (K == 1 ? pd.n_agents > 64 : pd.n_agents <= 64) return;
    P p;
    bind_doc(p, Q, pd, lds16, 1024ull * (uint64_t(pd.ne) + 16) + 4ull * pd.n_lv + (1u << 20));
    p.base = Q.base + pd.base_off;
    p.order = Q.order + pd.erec_off / EREC_WORDS;
    p.walk = Q.walk + 2 * size_t(d);
    res->n_tip = 0;
    if (p.ne > Q.lds_entries) {
        if (lane() == 0) res->status = PLAN_ERR_INTERNAL;
        return;
    }
    if constexpr (K == 1) plan_doc_split(p, res);
    else plan_doc<K>(p, res);
}

#ifndef DTGPU_PLAN_WAVES
#define DTGPU_PLAN_WAVES 6   // occupancy target of the <= 64-chain planner (tuning knob)
#endif
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(DTGPU_PLAN_WAVES))) void plan_kernel_1(PlanParams Q) {
    plan_entry<1>(Q);
}
__global__ __launch_bounds__(64) void plan_kernel_wide(PlanParams Q) { plan_entry<PLAN_MAX_AGENTS / 64>(Q); }


// ---- walk_kernel: the spanning-tree orders of CHAIN_WALK_DOCS documents per wave ----------------
// plan_doc_split's phase A for <= 64-chain documents, each on a 16-lane group: the same stack
// (a flat LDS stack here: push at the top, pick = the top unless it is a merge and a non-merge is
// below, which then swaps places with it), the same pending counts, one record load per step.
// A walk is a sequential chain of dependent steps whose work is a few lane operations, so one
// document per wave left most issue slots to waiting; four share each instruction here.  The plan
// kernel then runs phase B from the stored order (PlanParams.walk: status, steps).
constexpr uint32_t WG = 16, WALK_DOCS = 64 / WG;
DEV uint32_t wsh(uint32_t v, uint32_t src) { return uint32_t(__shfl(int(v), int(src))); }
// s_waitcnt vmcnt(0) alone, inside the branch that loads: where the paths meet the compiler then
// sees nothing pending and places no wait of its own -- a wait there would also wait for the
// order store of the step before (vmcnt counts stores), a full memory round trip per 16 steps
DEV void walk_wait_vm() { __builtin_amdgcn_s_waitcnt(0x0F70); }
template <bool CSR>
__global__ __launch_bounds__(64) void walk_kernel(PlanParams Q) {
    extern __shared__ __attribute__((aligned(16))) uint16_t wl16[];
    const uint32_t l = lane(), g = l / WG, c = l % WG, base = g * WG;
    const uint32_t cap = Q.todo_cap ? Q.todo_cap : PLAN_TODO_CAP;   // stack slots (even)
    const uint32_t stride = cap + (Q.lds_entries + 1) / 2;   // u16 per group: stack, pending bytes
    uint16_t *todo = wl16 + g * stride;
    uint8_t *pend = reinterpret_cast<uint8_t *>(todo + cap);
    const uint32_t li = blockIdx.x * WALK_DOCS + g;
    bool on = li < Q.n_docs;
    const uint32_t d = on ? (Q.doc_list ? Q.doc_list[li] : li) : 0u;
    const PlanDesc pd = Q.docs[d];
    on = on && !pd.skip && pd.n_agents <= 64 && pd.ne <= Q.lds_entries;
    const uint32_t ne = on ? pd.ne : 0u;
    const uint32_t *erec = Q.erec + pd.erec_off;
    const uint32_t *child = Q.child + pd.child_off;
    const uint32_t *coff = CSR ? Q.coff + pd.coff_off : nullptr, *poff = CSR ? Q.poff + pd.poff_off : nullptr;
    uint32_t *order = Q.order + pd.erec_off / EREC_WORDS;
    uint32_t err = 0, top = 0, hw = 0;   // hw: the stack's high-water mark
    const uint32_t limit = uint32_t(min<uint64_t>(1024ull * (uint64_t(ne) + 16) + 4ull * pd.n_lv + (1u << 20), 0xFFFFFFF0ull));
    uint32_t steps = 0;
    const uint32_t below = (1u << c) - 1u;
    bool bad_np = false;
    for (uint32_t e = c; e < ne; e += WG) {
        const uint32_t np = CSR ? poff[e + 1] - poff[e] : erec[size_t(e) * EREC_HEAD + R_NP];
        if (np > 0x7Fu) bad_np = true;
        pend[e] = uint8_t(min(np, 0x7Fu) | (np >= 2 ? MERGE_BIT : 0));
    }
    if ((uint32_t(__ballot(bad_np) >> base) & 0xFFFFu) && on) err = PLAN_WIDE_MERGE;
    // roots, highest index first, so the lowest root ends on the top
    for (int cb = int((ne + WG - 1) / WG) - 1; cb >= 0 && !err; cb--) {
        const uint32_t e = uint32_t(cb) * WG + (WG - 1 - c);
        const bool root = e < ne && (CSR ? poff[e + 1] == poff[e] : erec[size_t(e) * EREC_HEAD + R_NP] == 0);
        const uint32_t m = uint32_t(__ballot(root) >> base) & 0xFFFFu;
        if (top + uint32_t(__popc(m)) > cap) { err = PLAN_TODO_FULL; break; }
        if (root) todo[top + uint32_t(__popc(m & below))] = uint16_t(e);
        top += uint32_t(__popc(m));
        hw = max(hw, top);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    uint32_t ns = 0, ordv = 0;
    uint32_t wb = 0xFFFFFFFFu;   // CSR: the 64 entries whose records the group holds
    uint2 wk[4] = {};
    bool act = on && !err && top > 0;
    while (__ballot(act)) {
        if (act) {
            if (++steps > limit) { err = PLAN_ERR_INTERNAL; act = false; }
        }
        if (act) {
            // pick: the top, unless it is a merge and a non-merge lies below (it takes its place)
            const uint32_t t = top - 1;
            uint32_t idx = todo[t];
            if (pend[idx] & MERGE_BIT) {
                int found = -1;
                for (int hi = int(t) - 1; hi >= 0 && found < 0; hi -= int(WG)) {
                    const int i = hi - int(c);
                    const bool okk = i >= 0 && !(pend[todo[i]] & MERGE_BIT);
                    const uint32_t m = uint32_t(__ballot(okk) >> base) & 0xFFFFu;
                    if (m) found = hi - (__ffs(int(m)) - 1);
                }
                if (found >= 0) {
                    const uint32_t x = todo[found];
                    __builtin_amdgcn_wave_barrier();
                    if (c == 0) todo[found] = uint16_t(idx);
                    idx = x;
                }
            }
            top = t;
            ordv = c == (ns & (WG - 1)) ? idx : ordv;
            if ((ns & (WG - 1)) == WG - 1) order[ns - (WG - 1) + c] = ordv;
            ns++;
            // the entry's children (first / last from the record; a longer list from the CSR)
            uint32_t nch, ch0, firstch = 0, lastch = 0;
            if (CSR) {   // prep's first half: {children | first slot << 16, first | last child << 16}
                // the records of 64 consecutive entries stay in the group's lanes (lane c, word j:
                // entry wb + 16 j + c): a walk mostly steps to a nearby later entry, so few steps
                // load (friendsforever: 5 % of steps miss a 64-entry window, 19 % a 16-entry one,
                // and four documents share each wave's stall)
                if ((idx & ~63u) != wb) {
                    wb = idx & ~63u;
                    const uint2 *k2 = reinterpret_cast<const uint2 *>(coff);
#pragma unroll
                    for (uint32_t j = 0; j < 4; j++) wk[j] = k2[min(wb + WG * j + c, ne - 1)];
                    walk_wait_vm();
                }
                const uint32_t o = idx - wb, j = o / WG;   // group-uniform: each lane picks the word
                const uint2 v = j == 0 ? wk[0] : j == 1 ? wk[1] : j == 2 ? wk[2] : wk[3];
                const uint32_t src = base + (o & (WG - 1));
                const uint32_t w0 = wsh(v.x, src), w1 = wsh(v.y, src);
                nch = w0 & 0xFFFFu; ch0 = w0 >> 16; firstch = w1 & 0xFFFFu; lastch = w1 >> 16;
            } else {
                const uint32_t wsel = c == 0 ? R_NCH : c == 1 ? R_CH0 : c == 2 ? R_FIRSTCH : R_LASTCH;
                const uint32_t rv = erec[erec_word(ne, idx, wsel)];
                nch = wsh(rv, base); ch0 = wsh(rv, base + 1); firstch = wsh(rv, base + 2); lastch = wsh(rv, base + 3);
            }
            for (uint32_t cc = 0; cc < nch; cc += WG) {
                const bool has = cc + c < nch;
                uint32_t chv = nch <= 2 ? (c == 0 ? firstch : lastch) : 0u;
                if (has && nch > 2) {
                    chv = child[ch0 + cc + c];
                    walk_wait_vm();
                }
                bool ready = false;
                if (has) {
                    const uint8_t pdv = uint8_t(pend[chv] - 1);
                    pend[chv] = pdv;
                    ready = (pdv & 0x7F) == 0;
                }
                const uint32_t m = uint32_t(__ballot(ready) >> base) & 0xFFFFu;
                if (top + uint32_t(__popc(m)) > cap) { err = PLAN_TODO_FULL; break; }
                if (ready) todo[top + uint32_t(__popc(m & below))] = uint16_t(chv);
                top += uint32_t(__popc(m));
                hw = max(hw, top);
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            act = !err && top > 0;
        }
    }
    if (on && (ns & (WG - 1)) && c < (ns & (WG - 1))) order[(ns & ~(WG - 1)) + c] = ordv;
    if (on && c == 0) {
        Q.walk[2 * size_t(d)] = err | (hw << 16);   // status | stack high-water mark << 16
        Q.walk[2 * size_t(d) + 1] = ns;
    }
}

// ---- plan_kernel_xf: iter_xf_operations_from(from, merging) over a projected history ------------
//
// The document is the projection of Hist(from u merging) (dt_history.hip, entries kept as the base
// document's), the merged frontier is its tip.  build_xf_plan_from (dt_host.cpp) in the planner's
// terms: with vF the version vector of `from`, entry e of chain c has its first
// clamp(vF[c] - seq0, 0, len) LVs in Hist(from) -- its A part; the rest is its B part.
//   phase A   the spanning-tree walk over the A parts from ROOT, then one move to `from`: replayed,
//             not reported (PlanResult.xf_first = the first reported command);
//   prefix    B parts in ascending LV order while the part's parents are the frontier
//             (merge.rs:792-835): applied with no move;
//   phase B   the spanning-tree walk over the B parts that are left, then the move to the tip.
// A parent is consumed before phase B when it lies in an A part (pcnt <= vF[pch]) or below the
// prefix's bound; phase B counts only the other parents.  The B part of an entry with an A part
// has the one parent start - 1, consumed: it is a root of phase B, and no merge.
struct XS {
    uint32_t n_rep;      // reported LVs so far
    uint32_t rep;        // commands pushed now are reported
};
// (vc clamped into the entry's seq range first, then the subtraction: no operand of it can wrap)
DEV uint32_t a_len(uint32_t vc, uint32_t seq0, uint32_t len) {
    const uint32_t hi = seq0 + len;
    const uint32_t v = vc < seq0 ? seq0 : vc > hi ? hi : vc;
    return v - seq0;
}
// vF of a chain chosen per lane (lane = chain in vF).  All 64 lanes must be active.
DEV uint32_t vf_of(const VV<1> &vF, uint32_t ch) { return shfl(vF.v[0], ch & 63u); }
DEV void xrow(const P &p, uint32_t e, VV<1> &row) {
    const uint32_t l = lane();
    row.v[0] = l < p.A ? p.prow[size_t(e) * p.row_stride + l] : 0u;
}
// The entry holding lv (lv < n_lv): the last entry whose start is <= lv.
DEV uint32_t entry_of_lv(const P &p, uint32_t lv) {
    uint32_t lo = 0, hi = p.ne;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (U(p.erec[size_t(mid) * EREC_HEAD + R_START]) <= lv) lo = mid; else hi = mid;
    }
    return lo;
}
// Version vector of {lv}; chain and count of lv itself in c, n.
DEV void xvv_at(P &p, uint32_t lv, VV<1> &row, uint32_t &c, uint32_t &n) {
    const uint32_t e = entry_of_lv(p, lv);
    const uint32_t rw = load_rec(p, e);
    xrow(p, e, row);
    c = R(rw, R_CHAIN);
    n = R(rw, R_SEQ0) + (lv - R(rw, R_START)) + 1;
    fold_entry<1>(p, R(rw, R_START), R(rw, R_END), lv, c, R(rw, R_SEQ0), row, false);
}
// The entry's op runs clipped to the LVs [s, t) (truncate_tagged_span; XfPlanner::apply).
DEV void xapply(P &p, XS &x, uint32_t op0, uint32_t nop, uint32_t s, uint32_t t) {
    const uint32_t l = lane();
    for (uint32_t j0 = 0; j0 < nop && !p.err; j0 += 64) {
        const uint32_t j = j0 + l;
        Cmd c{0, 0, 0, 0};
        if (j < nop) c = p.opc[op0 + j];
        const uint32_t lo = max(c.lv, s), hi = min(c.lv + c.len, t);
        const bool inc = j < nop && lo < hi;
        const u64 m = __ballot(inc);
        const uint32_t cnt = uint32_t(__popcll(m));
        if (uint64_t(p.nc) + cnt > p.ccap) { fail(p, PLAN_CMDS_FULL); return; }
        if (inc && !p.count_only) {
            const uint32_t k = lo - c.lv, mm = hi - lo;
            const uint32_t pos = (c.op & 15u) == CMD_INS ? c.pos + k : (c.op & 16u) ? c.pos : c.pos + c.len - k - mm;
            p.cmds[p.nc + uint32_t(__popcll(m & ((1ull << l) - 1ull)))] = Cmd{c.op, lo, mm, pos};
        }
        p.nc += cnt;
        const uint32_t tot = rdl(scan_incl(inc ? hi - lo : 0u), 63);
        if (x.rep) x.n_rep += tot;
    }
}
// One of the two walks.  PB = false: the A parts from ROOT.  PB = true: the B parts that start
// at or above `bound` (the first LV the prefix did not consume).  vf: the tracker's version.
template <bool PB>
DEV void xwalk(P &p, XS &x, uint32_t bound, VV<1> &vf, const VV<1> &vF, const VV<1> &dlo, const VV<1> &dhi) {
    const uint32_t l = lane();
    const uint32_t *H = p.erec;
    uint32_t top = 0;
    for (uint32_t c0 = 0; c0 < p.ne; c0 += 64) {
        const uint32_t e = c0 + l;
        const bool valid = e < p.ne;
        const uint32_t *h = H + size_t(valid ? e : 0u) * EREC_HEAD;
        const uint32_t st = h[R_START], len = h[R_END] - st, np = h[R_NP], ch = h[R_CHAIN], po = h[R_POFF];
        const uint32_t vc = vf_of(vF, ch);
        const uint32_t al = ch < p.A ? a_len(vc, h[R_SEQ0], len) : 0u;
        uint32_t pend = np;
        bool in = valid && al > 0, mg = np >= 2;
        if (PB) {
            in = valid && al < len && st + al >= bound;
            // the parents that are not consumed yet (every lane steps together: vf_of)
            const uint32_t cnt = in && al == 0 ? np : 0u;
            uint32_t left = 0;
            for (uint32_t j = 0; __ballot(j < cnt) != 0; j++) {
                const bool on = j < cnt;
                const uint32_t pc = on ? p.pch[po + j] : 0u;
                const uint32_t vpc = vf_of(vF, pc);
                if (on) {
                    const bool done = (pc < p.A && p.pcnt[po + j] <= vpc) || p.par[po + j] < bound;
                    left += done ? 0u : 1u;
                }
            }
            if (al > 0) { pend = 0; mg = false; }
            else pend = left;
        }
        // (an entry outside this walk: 0x7F without the merge bit, which no entry of the walk holds --
        // a non-merge has at most one parent -- and which never reaches zero: it is never decremented)
        if (valid) p.pending[e] = in ? pend_byte(pend, mg) : uint8_t(0x7F);
    }
    seed_roots(p, top);
    while (top > 0 && !p.err) {
        if (!charge(p)) break;
        const uint32_t idx = pick(p, top);
        const uint32_t rw = load_rec(p, idx);
        const uint32_t st = R(rw, R_START), en = R(rw, R_END), op0 = R(rw, R_OP0), nop = R(rw, R_NOP),
                       ch0 = R(rw, R_CH0), nch = R(rw, R_NCH), chain = R(rw, R_CHAIN), seq0 = R(rw, R_SEQ0);
        if (chain >= p.A || en <= st) { fail(p, PLAN_ERR_INTERNAL); break; }
        const uint32_t al = a_len(rdl(vF.v[0], chain), seq0, en - st);
        const uint32_t s = PB ? st + al : st, t = PB ? en : st + al;
        if (s >= t) { fail(p, PLAN_ERR_INTERNAL); break; }
        // the part's parents: the entry's, or (a B part behind an A part) the LV before it
        VV<1> vp;
        xrow(p, idx, vp);
        if (l == chain) vp.v[0] = max(vp.v[0], seq0 + (s - st));
        move_to<1>(p, vf, vp, dlo, dhi, true);
        if (p.err) break;
        xapply(p, x, op0, nop, s, t);
        if (p.err) break;
        vf = vp;
        if (l == chain) vf.v[0] = seq0 + (t - st);
        // children whose last counted parent this part held (pushed in child index order)
        for (uint32_t c = 0; c < nch; c += 64) {
            bool ready = false;
            const bool valid = c + l < nch;
            const uint32_t chv = valid ? p.child[ch0 + c + l] : 0u;
            const uint32_t *h = H + size_t(chv) * EREC_HEAD;
            const uint32_t cst = h[R_START], cch = h[R_CHAIN];
            const uint32_t cvc = vf_of(vF, cch);
            const uint32_t cal = cch < p.A ? a_len(cvc, h[R_SEQ0], h[R_END] - cst) : 0u;
            if (valid) {
                bool dec = cal > 0;
                if (PB) {   // counted iff the child has no A part and its parent here lies in this part
                    dec = false;
                    const uint32_t po = h[R_POFF], np = h[R_NP];
                    for (uint32_t j = 0; j < np && cal == 0; j++) {
                        const uint32_t pl = p.par[po + j];
                        if (pl >= st && pl < en) { dec = pl >= s; break; }
                    }
                }
                if (dec) {
                    const uint8_t pd = uint8_t(p.pending[chv] - 1);
                    p.pending[chv] = pd;
                    ready = (pd & 0x7F) == 0;
                }
            }
            if (!push_ready(p, top, ready, chv)) break;
        }
        fence_wave();
    }
}

DEV void plan_doc_xf(P &p, XS &x, const uint32_t *from, uint32_t n_from, PlanResult *res) {
    const uint32_t l = lane();
    VV<1> vf, vF, dlo, dhi;
    vv_zero(vf);
    vv_zero(vF);
    dlo.v[0] = l < p.A ? p.doff[l] : 0;
    dhi.v[0] = l < p.A ? p.doff[l + 1] : 0;
    bool bad_np = false;   // a parent count past the pending byte: as the whole-document planner
    for (uint32_t e = l; e < p.ne; e += 64) bad_np |= p.erec[size_t(e) * EREC_HEAD + R_NP] > 0x7Fu;
    if (__ballot(bad_np)) fail(p, PLAN_WIDE_MERGE);
    // vF, and `from` reduced to a frontier (lane j: its j-th LV, ascending as given): an LV is
    // dominated when another one's history reaches it on its chain.  Serial over the set, quadratic
    // for the LVs that end their chain's part of it: the caller bounds the set (MERGE_MAX_FROM)
    for (uint32_t j = 0; j < n_from && !p.err; j++) {
        if (!charge(p)) break;
        const uint32_t lv = U(from[j]);
        if (lv >= p.n_lv) { fail(p, PLAN_ERR_INTERNAL); break; }
        VV<1> t;
        uint32_t c, n;
        xvv_at(p, lv, t, c, n);
        vv_max(vF, t);
    }
    uint32_t fr = 0, nfr = 0;
    for (uint32_t j = 0; j < n_from && !p.err; j++) {
        if (!charge(p)) break;
        const uint32_t lv = U(from[j]);
        VV<1> t;
        uint32_t c, n;
        xvv_at(p, lv, t, c, n);
        bool dom = rdl(vF.v[0], c) > n;   // a later LV of its chain is in Hist(from)
        for (uint32_t k = 0; k < n_from && !dom && !p.err; k++) {
            if (!charge(p)) break;
            const uint32_t lk = U(from[k]);
            if (lk == lv) { dom = k < j; continue; }   // a repeat counts once
            VV<1> tk;
            uint32_t ck, nk;
            xvv_at(p, lk, tk, ck, nk);
            dom = rdl(tk.v[0], c) >= n;
        }
        if (!dom) {
            if (nfr >= 64) { fail(p, PLAN_ERR_INTERNAL); break; }
            if (l == nfr) fr = lv;
            nfr++;
        }
    }
    tk(p);
    // phase A: Hist(from), then the tracker at `from`
    x.rep = 0;
    if (!p.err && n_from) xwalk<false>(p, x, 0, vf, vF, dlo, dhi);
    if (!p.err) move_to<1>(p, vf, vF, dlo, dhi, true);
    vf = vF;
    const uint32_t first = p.nc;
    x.rep = 1;
    // the fast-forward prefix: B parts in LV order while their parents are the frontier
    uint32_t bound = p.n_lv;
    bool single = false;   // the frontier is the one LV f (else: `from`, fr / nfr)
    uint32_t f = 0;
    for (uint32_t e = 0; e < p.ne && !p.err; e++) {
        if (!charge(p)) break;
        {   // skip, 64 at a time, the entries that lie in Hist(from) whole
            const uint32_t k = e + l;
            const uint32_t *h = p.erec + size_t(k < p.ne ? k : 0u) * EREC_HEAD;
            const uint32_t len = h[R_END] - h[R_START], ch = h[R_CHAIN];
            const uint32_t vc = vf_of(vF, ch);
            const bool part = k < p.ne && (ch >= p.A || a_len(vc, h[R_SEQ0], len) < len);
            const u64 m = __ballot(part);
            if (!m) { e += 63; continue; }
            e += ctz(m);
        }
        const uint32_t rw = load_rec(p, e);
        const uint32_t st = R(rw, R_START), en = R(rw, R_END), chain = R(rw, R_CHAIN), seq0 = R(rw, R_SEQ0),
                       np = R(rw, R_NP), po = R(rw, R_POFF);
        if (chain >= p.A) { fail(p, PLAN_ERR_INTERNAL); break; }
        const uint32_t al = a_len(rdl(vF.v[0], chain), seq0, en - st);
        if (al == en - st) continue;   // all of it in Hist(from)
        const uint32_t s = st + al;
        bool same;
        if (al > 0) {
            same = single ? f == s - 1 : (nfr == 1 && rdl(fr, 0) == s - 1);
        } else if (single) {
            same = np == 1 && R(rw, R_PAR0) == f;
        } else {   // the parents and `from`: two reduced frontiers of equal size, one inside the other
            same = np == nfr;
            for (uint32_t j = 0; j < np && same; j++) {
                const uint32_t pl = U(p.par[po + j]);
                same = __ballot(l < nfr && fr == pl) != 0;
            }
        }
        if (!same) { bound = s; break; }
        xapply(p, x, R(rw, R_OP0), R(rw, R_NOP), s, en);
        if (l == chain) vf.v[0] = seq0 + (en - st);
        single = true;
        f = en - 1;
    }
    // phase B: what is left, then the merged version
    if (!p.err && bound < p.n_lv) xwalk<true>(p, x, bound, vf, vF, dlo, dhi);
    if (!p.err) {
        VV<1> vt;
        vv_zero(vt);
        for (uint32_t j = 0; j < p.ntip && !p.err; j++) {
            const uint32_t lv = U(p.tip[2 * j]);
            if (lv >= p.n_lv) { fail(p, PLAN_ERR_INTERNAL); break; }
            VV<1> t;
            uint32_t c, n;
            xvv_at(p, lv, t, c, n);
            vv_max(vt, t);
        }
        move_to_tip<1>(p, res, vf, vt, dlo, dhi, true);
    }
    write_result(p, res);
    if (l == 0) { res->xf_first = first; res->n_xf = x.n_rep; }
}

__global__ __launch_bounds__(64) void plan_kernel_xf(PlanParams Q) {
    extern __shared__ __attribute__((aligned(16))) uint16_t lds16[];
    if (blockIdx.x >= Q.n_docs) return;
    const uint32_t d = U(Q.doc_list ? Q.doc_list[blockIdx.x] : blockIdx.x);
    const PlanDesc pd = Q.docs[d];
    PlanResult *res = Q.results + d;
    if (pd.skip) return;
    P p;
    bind_doc(p, Q, pd, lds16, 2048ull * (uint64_t(pd.ne) + 16) + 4ull * pd.n_lv + 4ull * uint64_t(pd.n_from) * pd.n_from + (1u << 20));
    XS x{0, 0};
    res->n_tip = 0;
    if (p.ne > Q.lds_entries || p.A > 64 || p.ne == 0) {
        if (lane() == 0) res->status = PLAN_ERR_INTERNAL;
        return;
    }
    plan_doc_xf(p, x, Q.xf_from + pd.xf_off, U(pd.n_from), res);
}

}  // namespace pdev

int launch_walk(const PlanParams &q, void *stream, bool csr) {
    if (!q.n_docs) return OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t cap = q.todo_cap ? q.todo_cap : PLAN_TODO_CAP;
    if (cap > PLAN_TODO_CAP || (cap & 1u)) return ErrArg;
    const size_t wlds = size_t(pdev::WALK_DOCS) * 2 * (cap + (q.lds_entries + 1) / 2);
    const dim3 grid((q.n_docs + pdev::WALK_DOCS - 1) / pdev::WALK_DOCS);
    if (wlds > 160 * 1024) return ErrArg;
    if (wlds > 64 * 1024) {   // past the default dynamic-LDS limit (documents near PLAN_MAX_LDS_ENTRIES)
        const void *fn = csr ? reinterpret_cast<const void *>(&pdev::walk_kernel<true>) : reinterpret_cast<const void *>(&pdev::walk_kernel<false>);
        if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, int(160 * 1024)) != hipSuccess) return ErrHip;
    }
    if (csr) hipLaunchKernelGGL(pdev::walk_kernel<true>, grid, dim3(64), wlds, s, q);
    else hipLaunchKernelGGL(pdev::walk_kernel<false>, grid, dim3(64), wlds, s, q);
    return launch_error() == hipSuccess ? OK : ErrHip;
}

int launch_plan(const PlanParams &q, void *stream, bool walk) {
    if (!q.n_docs) return OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = 2 * size_t(PLAN_TODO_CAP) + ((size_t(q.lds_entries) + 15) & ~size_t(15));   // todo + pending
    if (q.xf) {   // merge requests over projected histories
        hipLaunchKernelGGL(pdev::plan_kernel_xf, dim3(q.n_docs), dim3(64), lds, s, q);
        return launch_error() == hipSuccess ? OK : ErrHip;
    }
    if (walk && launch_walk(q, stream, false)) return ErrHip;
    hipLaunchKernelGGL(pdev::plan_kernel_1, dim3(q.n_docs), dim3(64), lds, s, q);
    if (launch_error() != hipSuccess) return ErrHip;
    if (q.max_agents > 64) {
        hipLaunchKernelGGL(pdev::plan_kernel_wide, dim3(q.n_docs), dim3(64), lds, s, q);
        if (launch_error() != hipSuccess) return ErrHip;
    }
    return OK;
}

}  // namespace dtgpu
