// dtgpu_stage.cpp -- batch staging: a batch's documents laid out in HBM.  Two front ends -- stage()
// (host decode, planner arrays uploaded) and stage_device() (device decode, planner arrays built by
// the prep kernel) -- meet in one layout: the planner's sizing pass, a document's fast-forward or
// tracker layout, the segments, the arenas and the replay tiers' parameters.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dt_batch.hpp"
#include "dt_merge.hpp"

namespace dtgpu {

Settings settings_for(const dtgpu_batch_opts *o) {
    Settings c;
    if (o) {
        c.ff = !(o->flags & DTGPU_OPT_NO_FAST_FORWARD);
        c.seg = !(o->flags & DTGPU_OPT_NO_SEGMENTS);
        c.host_plan = (o->flags & DTGPU_OPT_HOST_PLAN) != 0;
        c.split = !(o->flags & DTGPU_OPT_NO_SPLIT);
        c.critical = !(o->flags & DTGPU_OPT_NO_CRITICAL);
        c.debug = (o->flags & DTGPU_OPT_DEBUG) ? 1u : 0u;
        c.pass_mark = (o->flags & DTGPU_OPT_PASS_MARK) != 0;
        c.blame = (o->flags & DTGPU_OPT_BLAME) != 0;
        if (o->seg_ops) c.seg_ops = o->seg_ops;
        if (o->seg_max) c.seg_max = o->seg_max;
        if (o->lds_fill) c.lds_fill = o->lds_fill;
    }
    auto on = [](const char *name, bool &v) { if (const char *e = getenv(name)) v = *e != '0'; };
    auto set = [](const char *name) { return getenv(name) != nullptr; };
    auto num = [](const char *name, uint64_t lo, uint64_t hi, uint64_t &v) {
        if (const char *e = getenv(name)) v = std::min<uint64_t>(std::max<uint64_t>(lo, strtoull(e, nullptr, 10)), hi);
    };
    on("DTGPU_FF", c.ff);
    on("DTGPU_SEG", c.seg);
    num("DTGPU_SEG_OPS", 1, UINT64_MAX, c.seg_ops);
    uint64_t x = c.seg_max; num("DTGPU_SEG_MAX", 1, 64, x); c.seg_max = uint32_t(std::min<uint64_t>(x, 64));
    x = c.seg_w; num("DTGPU_SEG_W", 0, 1u << 20, x); c.seg_w = uint32_t(x);
    on("DTGPU_SEG_FAIR", c.seg_fair);
    on("DTGPU_SEG_LATE", c.seg_late);
    on("DTGPU_LATE_PIPE", c.late_pipe);
    num("DTGPU_LATE_FROM", 1, UINT64_MAX, c.late_from);
    num("DTGPU_LDS_FILL", 1, UINT64_MAX, c.lds_fill);
    on("DTGPU_FLAT", c.flat);
    on("DTGPU_PREP_CHAINS", c.prep_chains);
    on("DTGPU_CRITICAL", c.critical);
    on("DTGPU_PRIO", c.prio);
    if (set("DTGPU_HOST_PLAN")) c.host_plan = true;
    if (set("DTGPU_NO_SPLIT")) c.split = false;
    if (set("DTGPU_NO_FALLBACK")) c.fallback = false;
    if (set("DTGPU_NO_WALK_OVERLAP")) c.walk_overlap = false;
    if (const char *e = getenv("DTGPU_DEBUG")) c.debug = uint32_t(atoi(e) ? atoi(e) : 1);
    c.prep_check = c.debug != 0 || set("DTGPU_PREP_CHECK");
    if (set("DTGPU_PASS_MARK")) c.pass_mark = true;
    c.plan_prof = set("DTGPU_PLAN_PROF");
    c.enc_prof = set("DTGPU_ENC_PROF");
    x = c.tog_waves; num("DTGPU_TOG_WAVES", 0, 64, x); c.tog_waves = uint32_t(x);
    x = c.tog_mw_lds; num("DTGPU_TOG_MW_LDS", 0, UINT64_MAX, x); c.tog_mw_lds = uint32_t(std::min<uint64_t>(x, UINT32_MAX));
    x = 0; num("DTGPU_ENC_LDS_TEXT", 0, 24064, x); c.enc_lds_text = uint32_t(x);
    // a blame batch is another product than the headline: one pipeline, and cuts only where a
    // document is long (every uncut document is a segment group of one, dt_blame.hpp)
    if (c.blame) c.late_pipe = c.seg_late = false;
    return c;
}

namespace {

template <typename T>
void append(std::vector<T> &dst, const std::vector<T> &src) { dst.insert(dst.end(), src.begin(), src.end()); }

constexpr uint64_t kItemTierCap[kLdsTiers] = {12 * 1024, 32 * 1024, 64 * 1024, 160 * 1024};
int item_tier(uint32_t est) {
    const uint64_t bytes = index_bytes_ms(est, lds_sb_capacity(est), true);
    for (int t = 0; t < kLdsTiers; t++) if (bytes <= kItemTierCap[t]) return t;
    return -1;
}
Layout replay_layout(uint64_t n_ins, uint64_t lds_fill, bool hbm_only) {
    Layout L{};
    L.max_blocks = uint32_t(n_ins / 32 + 2);
    L.gidx = index_bytes(L.max_blocks);
    const uint32_t est = uint32_t(std::min<uint64_t>(L.max_blocks, n_ins / lds_fill + 8));
    L.tier = hbm_only ? -1 : item_tier(est);
    L.tier_blocks = est;
    return L;
}
SegSettings seg_settings(const Settings &c) {
    return SegSettings{c.seg, c.seg_ops, std::min<uint32_t>(c.seg_max, 64), c.seg_w};   // (<= 64: the device cut planning's lane per segment)
}

// ---- what the two stagings share -------------------------------------------------------------
// What the layout needs to know of one decoded document, whichever side decoded it.
struct DocFacts {
    uint64_t n_lv, n_ops, n_entries, n_parents, n_aruns, n_content, n_ins;   // n_content: inserted bytes; n_ins: chars
    bool linear;   // one graph entry, with ops and all its content: it can fast-forward (dt_ff.hip)
};
DocFacts facts_of(const HostOpLog &o) {
    DocFacts f{};
    f.n_lv = o.n_lv;
    f.n_ops = o.ops.size();
    f.n_entries = o.graph.entries.size();
    for (const GraphEntry &g : o.graph.entries) f.n_parents += g.parents.size();
    f.n_aruns = o.agent_runs.size();
    f.n_content = o.ins_content.size();
    for (const OpRun &r : o.ops) if (r.kind == 0) f.n_ins += r.len;
    f.linear = f.n_entries == 1 && f.n_ops > 0 && o.content_complete;
    return f;
}
DocFacts facts_of(const DecodeResult &r, const PrepResult &p) {
    return DocFacts{r.n_lv, r.n_ops, r.n_entries, r.n_parents, r.n_aruns, r.n_content, p.n_ins,
                    r.n_entries == 1 && r.n_ops > 0 && r.content_complete};
}
// The running sizes of the batch's arenas while its documents are laid out.
struct Totals { uint64_t cmd = 0, tlist = 0, lv = 0, pc = 0, blk = 0, out = 0, gidx = 0, src = 0; };

// Compulsory input bytes of the decoded oplog (SURVEY.md §8d merge-only formula): 16 per op run +
// (8 + 4 per parent) per graph entry + 12 per agent run + inserted bytes; the text written is
// added from the results (dtgpu_batch_algorithmic_bytes).
uint64_t alg_in_bytes(const DocFacts &f) {
    return 16ull * f.n_ops + 8ull * f.n_entries + 4ull * f.n_parents + 12ull * f.n_aruns + f.n_content;
}
// More inserted chars than a document's block arena can index (-> ErrCapacity).
bool over_block_limit(uint64_t n_ins) { return n_ins / 32 + 2 > std::min<uint64_t>(LOC_MAX_BLOCKS, MAX_DOC_BLOCKS); }

// A new batch of n documents on B.device: the device's CU count, the per-document vectors.
dtgpu_status begin_batch(dtgpu_batch &B, size_t n) {
    DTGPU_CK(hipSetDevice(B.device));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, B.device) == hipSuccess && prop.multiProcessorCount > 0)
        B.n_cu = prop.multiProcessorCount;
    B.n = n;
    B.host_status.assign(n, OK);
    B.n_lv.assign(n, 0);
    B.n_runs.assign(n, 0);
    B.docs.assign(n, DocDesc{});
    B.host_planned.assign(n, 0);
    B.ff_doc.assign(n, 0);
    return DTGPU_OK;
}
void reset_doc(DocDesc &d) {
    std::memset(&d, 0, sizeof d);
    d.seg_hi = 0xFFFFFFFFu;   // not a segment (cut replay)
    d.src_off = ~0ull;
}
// A device-planned document's command and tlist slots, as the sizing pass counted them.
void plan_slots(dtgpu_batch &B, DocDesc &d, PlanDesc &q, const PlanResult &r, Totals &T) {
    d.cmd_off = T.cmd; d.tlist_off = T.tlist;
    d.ncmd = r.ncmd;
    q.cmd_off = T.cmd; q.tlist_off = T.tlist;
    q.ccap = r.ncmd; q.tcap = r.ntlist;
    T.cmd += r.ncmd;
    T.tlist += r.ntlist;
    B.n_gpu_planned++;
}
void describe(DocDesc &d, const DocFacts &f) {
    d.ascii = f.n_content == f.n_ins ? 1u : 0u;
    d.n_lv = uint32_t(f.n_lv);
    d.content_len = uint32_t(f.n_content);
}
// A linear history: the fast-forward path (dt_ff.hip), out arena only (16-byte aligned).
void layout_ff_doc(dtgpu_batch &B, size_t i, const DocFacts &f, Totals &T) {
    DocDesc &d = B.docs[i];
    B.ff_doc[i] = 1;
    d.flags |= DOC_FF;
    T.out = (T.out + 15) & ~15ull;
    d.out_off = T.out;
    d.out_cap = uint32_t(f.n_content);
    T.out += (uint64_t(d.out_cap) + 15) & ~15ull;
    B.alg_in_bytes += alg_in_bytes(f);
}
// A tracker document: blocks, out and HBM index arenas and its replay tier, which is returned
// (-1: the HBM tier).  Every document gets an HBM index (the LDS tier hands back documents that
// outgrow their optimistic LDS capacity); the LDS tier is sized from the expected block fill
// (Settings::lds_fill).
int layout_tracker_doc(dtgpu_batch &B, size_t i, const DocFacts &f, bool hbm_only, Totals &T) {
    DocDesc &d = B.docs[i];
    const Layout lay = replay_layout(f.n_ins, B.cfg.lds_fill, hbm_only);
    d.max_blocks = lay.max_blocks;
    d.blk_off = T.blk;
    d.out_off = T.out;
    d.out_cap = uint32_t(f.n_content);
    d.gidx_off = T.gidx;
    T.blk += d.max_blocks;
    T.out += d.out_cap;
    T.gidx += lay.gidx;
    B.alg_in_bytes += alg_in_bytes(f);
    if (lay.tier >= 0) {
        B.tier_list[lay.tier].push_back(uint32_t(i));
        B.tier_blocks[lay.tier] = std::max(B.tier_blocks[lay.tier], lay.tier_blocks);
    } else {
        B.large_list.push_back(uint32_t(i));
    }
    return lay.tier;
}

// The planner's sizing pass over the batch's planner arrays: its scratch, PlanParams (the caller
// has set what differs between the stagings: prow, coff, poff), one count-only launch, and the
// per-document counts read back -- with `wres`, the walk kernel's {status, steps} words too.
dtgpu_status size_plans(dtgpu_batch &B, const std::vector<PlanDesc> &pdesc, uint64_t erec_words, uint32_t lds_entries,
                        uint32_t max_agents, std::vector<PlanResult> &pres, std::vector<uint32_t> *wres) {
    const size_t n = B.n;
    hipStream_t s = B.stream;
    DTGPU_CK(B.p_order.alloc(std::max<uint64_t>(erec_words / EREC_WORDS, 1)));
    DTGPU_CK(B.p_walk.alloc(2 * std::max<size_t>(n, 1)));
    DTGPU_CK(B.p_docs.upload(pdesc, s));
    DTGPU_CK(B.p_results.alloc(n));
    DTGPU_CK(hipMemsetAsync(B.p_results.p, 0, std::max<size_t>(n, 1) * sizeof(PlanResult), s));
    PlanParams &q = B.plan;
    q.par = B.p_par.p; q.pent = B.p_pent.p; q.pch = B.p_pch.p; q.pcnt = B.p_pcnt.p;
    q.child = B.p_child.p; q.opc = B.p_opc.p;
    q.aruns = B.d_aruns.p; q.tip = B.p_tip.p; q.erec = B.p_erec.p; q.doff = B.p_doff.p;
    q.dense = B.p_dense.p; q.base = B.p_base.p; q.order = B.p_order.p;
    q.walk = B.p_walk.p;
    q.lds_entries = (lds_entries + 7) & ~7u;
    q.max_agents = max_agents;
    q.prof = B.cfg.plan_prof ? 1u : 0u;
    q.docs = B.p_docs.p; q.results = B.p_results.p; q.n_docs = uint32_t(n);
    q.count_only = 1;
    q.todo_cap = 0;
    if (launch_plan(q, s) != OK) { DTGPU_HIP_FAILED(hipErrorLaunchFailure); return DTGPU_ERR_HIP; }
    q.count_only = 0;
    pres.resize(n);
    DTGPU_CK(hipMemcpyAsync(pres.data(), B.p_results.p, std::max<size_t>(n, 1) * sizeof(PlanResult), hipMemcpyDeviceToHost, s));
    if (wres) {
        wres->resize(2 * n);
        DTGPU_CK(hipMemcpyAsync(wres->data(), q.walk, 2 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    }
    DTGPU_CK(hipStreamSynchronize(s));
    return DTGPU_OK;
}

size_t n_lds_docs(const dtgpu_batch &B) {
    size_t k = 0;
    for (int t = 0; t < kLdsTiers; t++) k += B.tier_list[t].size();
    return k;
}
std::vector<uint32_t> segment_owners(const dtgpu_batch &B);
// Launch order of the documents: the LDS tiers, then the HBM tier; inside a list the documents
// go by descending LVs (a cut document's first segment by its own), so the hardware dispatcher
// starts the longest replays first (LPT inside the GPU: the short ones fill in behind them), the
// critical ones (DOC_CRITICAL) before all.
std::vector<uint32_t> tier_lists(dtgpu_batch &B) {
    std::vector<uint32_t> all;
    auto by_cost = [&](std::vector<uint32_t> &v) {
        auto cost = [&](uint32_t d) -> uint64_t {
            if (B.docs[d].flags & DOC_CRITICAL) return UINT64_MAX;   // the critical path first
            if (d >= B.n) return B.seg_cost[d - B.n];
            return d < B.first_cost.size() && B.first_cost[d] ? B.first_cost[d] : B.n_lv[d];
        };
        std::stable_sort(v.begin(), v.end(), [&](uint32_t a, uint32_t b) { return cost(a) > cost(b); });
    };
    for (int t = 0; t < kLdsTiers; t++) {
        std::vector<uint32_t> &v = B.tier_list[t];
        by_cost(v);
        if (t == 0 && B.late_pipe) {   // the first round's workgroups, then the late documents' (both halves of a cut one)
            const std::vector<uint32_t> owner = segment_owners(B);
            const auto mid = std::stable_partition(v.begin(), v.end(), [&](uint32_t d) { return !B.late_doc[owner[d]]; });
            B.flat_first = uint32_t(mid - v.begin());
        }
        append(all, v);
    }
    by_cost(B.large_list);
    append(all, B.large_list);
    return all;
}
// The replay tiers' parameters: the arenas (cbyte / content: the batch's uploads, or the
// decoder's arenas read in place), each tier's list and LDS sizing, the side streams.
dtgpu_status set_tier_params(dtgpu_batch &B, const uint32_t *cbyte, const uint8_t *content) {
    BatchParams base{};
    base.mup = B.d_mup.p;   // (transformed-ops batches only: null otherwise)
    base.tup = B.d_tup.p;
    base.xf = B.d_xf.p;
    base.debug = B.cfg.debug;
    base.cmds = B.d_cmds.p; base.tlist = B.d_tlist.p; base.aruns = B.d_aruns.p;
    base.cbyte = cbyte; base.content = content;
    base.pos = B.d_pos.p; base.ao = B.d_ao.p; base.items = B.d_items.p; base.m2 = B.d_m2.p;
    base.out = B.d_out.p; base.gidx = B.d_gidx.p; base.src = B.d_src.p;
    base.docs = B.d_docs.p; base.results = B.d_results.p;
    const bool fb = n_lds_docs(B) && B.cfg.fallback;
    size_t off = 0;
    for (int t = 0; t < kLdsTiers; t++) {
        BatchParams &q = B.tier[t];
        q = base;
        q.doc_list = B.d_lists.p + off;
        q.n_list = uint32_t(B.tier_list[t].size());
        q.lds_blocks = B.tier_blocks[t];
        q.lds_sb = lds_sb_capacity(q.lds_blocks);
        q.lds_flat = t == 0 && B.cfg.flat && q.lds_blocks <= FLAT_MAX_BLOCKS ? 1u : 0u;
        q.prio_on = B.cfg.prio ? 1u : 0u;
        q.tog_waves = B.cfg.tog_waves;
        q.tog_mw_lds = B.cfg.tog_mw_lds;
        off += B.tier_list[t].size();
        if (fb) { q.fb_count = B.d_fb.p; q.fb_list = B.d_fb.p + 1; }
    }
    B.large = base;
    B.large.doc_list = B.d_lists.p + off;
    B.large.n_list = uint32_t(B.large_list.size());
    if (fb) {
        B.large.fb_count = B.d_fb.p;
        B.large.fb_list = B.d_fb.p + 1;
        B.large.fb_slots = uint32_t(off);   // every LDS-tier document may be handed back
    }
    for (int t = 0; t < kLdsTiers; t++) B.tier[t].n_cu = uint32_t(B.n_cu);
    B.large.n_cu = uint32_t(B.n_cu);
    B.debug = base.debug;
    if (!B.ev_fork) DTGPU_CK(hipEventCreateWithFlags(&B.ev_fork, hipEventDisableTiming));
    if (!B.ev_splan) DTGPU_CK(hipEventCreateWithFlags(&B.ev_splan, hipEventDisableTiming));
    // the late pipeline's two streams at the lowest priority: whenever workgroups of both pipelines
    // wait for a slot, the first round's go first (its whole documents are the pass's critical path)
    int prio_least = 0, prio_greatest = 0;
    if (B.late_pipe) DTGPU_CK(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    for (int k = 0; k < kSideStreams; k++) {
        if (!B.side[k] && B.late_pipe && k < 2) DTGPU_CK(hipStreamCreateWithPriority(&B.side[k], hipStreamNonBlocking, prio_least));
        if (!B.side[k]) DTGPU_CK(hipStreamCreateWithFlags(&B.side[k], hipStreamNonBlocking));
        if (!B.ev_join[k]) DTGPU_CK(hipEventCreateWithFlags(&B.ev_join[k], hipEventDisableTiming));
    }
    return DTGPU_OK;
}

// Add document i's later segments (cuts[1..]) as documents of its replay tier (or the HBM
// tier) and make document i the first segment.
bool add_segments(dtgpu_batch &B, uint32_t i, const std::vector<SegCut> &cuts, int tier, Totals &T) {
    std::vector<uint32_t> mb(cuts.size(), 0);
    for (size_t k = 1; k < cuts.size(); k++) {
        // placeholders 48 per block, then the inserts -- and at least what the HBM tier's
        // midpoint splits guarantee (every block keeps >= 32 items, so (u + ins) / 32 + 2
        // blocks hold any placement of the inserts among the placeholders)
        const uint64_t m = std::max<uint64_t>((uint64_t(cuts[k].u) + 47) / 48 + cuts[k].ins / 32 + 3,
                                              (uint64_t(cuts[k].u) + cuts[k].ins) / 32 + 3);
        if (m > std::min<uint64_t>(LOC_MAX_BLOCKS, MAX_DOC_BLOCKS)) return false;
        mb[k] = uint32_t(m);
    }
    const SegGroup g{uint32_t(B.seg_docs.size()), uint32_t(cuts.size())};
    {
        DocDesc &d0 = B.docs[i];
        d0.seg_hi = cuts[0].hi;
        d0.src_off = T.src;
        d0.src_cap = uint32_t(cuts[0].ins);
        T.src += cuts[0].ins;
    }
    B.seg_docs.push_back(i);
    if (B.first_cost.size() < B.n) B.first_cost.resize(B.n, 0);
    B.first_cost[i] = std::max<uint64_t>(1, cuts[0].hi);
    const uint64_t n_lv = B.docs[i].n_lv;
    for (size_t k = 1; k < cuts.size(); k++) {
        DocDesc e = B.docs[i];
        e.seg_lo = cuts[k].lo;
        e.seg_hi = cuts[k].hi;
        e.seg_u = cuts[k].u;
        e.pc_off = T.pc;
        T.pc += n_lv + cuts[k].u;
        e.max_blocks = mb[k];
        e.blk_off = T.blk;
        T.blk += mb[k];
        e.gidx_off = T.gidx;
        T.gidx += index_bytes(mb[k]);
        e.src_off = T.src;
        e.src_cap = uint32_t(cuts[k].u + cuts[k].ins);
        T.src += e.src_cap;
        const uint32_t idx = uint32_t(B.docs.size());
        B.docs.push_back(e);
        B.seg_cost.push_back(cuts[k].hi == 0xFFFFFFFFu ? n_lv - cuts[k].lo : cuts[k].hi - cuts[k].lo);
        B.seg_docs.push_back(idx);
        // its own replay tier, sized for its placeholders and inserts, never above its
        // document's: a split pass replays the biggest tier beside the other documents' plans,
        // so a segment may sit there only when its document is planned there too (the main
        // stream waits for the big tier's plans before replaying any tier: see replay_all); a
        // document on the HBM tier keeps its segments there
        const Layout lay = replay_layout(cuts[k].u + cuts[k].ins, B.cfg.lds_fill, false);
        if (tier >= 0 && lay.tier >= 0 && lay.tier <= tier) {
            const uint32_t est = std::max<uint32_t>(lay.tier_blocks, uint32_t((uint64_t(cuts[k].u) + 47) / 48 + 8));
            B.tier_list[lay.tier].push_back(idx);
            B.tier_blocks[lay.tier] = std::max(B.tier_blocks[lay.tier], std::min(est, mb[k]));
        } else {
            B.large_list.push_back(idx);
        }
    }
    B.seg_groups.push_back(g);
    return true;
}
// Which documents of a batch replay as segments, and how long a segment is: a document is cut
// when it holds at least two segments' worth of op runs, where a segment is DTGPU_SEG_OPS op
// runs or the batch's fair share per wave slot (all op runs over 8 waves per CU), whichever is
// more -- a batch of many equal documents already fills the GPU and is left alone.
template <typename NOps>
std::vector<uint32_t> seg_candidates(size_t n, SegSettings &sc, int n_cu, bool fair, NOps n_ops) {
    std::vector<uint32_t> c;
    if (!sc.on) return c;
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++) total += n_ops(i);
    if (fair) sc.ops_per_seg = std::max<uint64_t>(sc.ops_per_seg, total / (uint64_t(std::max(n_cu, 1)) * 8));
    for (size_t i = 0; i < n; i++)
        if (n_ops(i) >= 2 * sc.ops_per_seg) c.push_back(uint32_t(i));
    return c;
}
// The documents the smallest LDS tier dispatches after its first resident round (its list runs
// longest first, so these are its shortest): they start when the first round's documents begin
// to finish and would run to the end of the batch at low occupancy; each is cut once where its
// history allows, so its two halves finish earlier beside each other.  (Device-staged batches:
// the pass itself plans the cut, cut_kernel.)
// The flat tier's documents longest first, and how many of them one resident round holds
// (DTGPU_LATE_FROM overrides the device's figure: a small test batch then has a late set).
struct FlatRounds { std::vector<uint32_t> order; size_t resident = 0; };
FlatRounds flat_rounds(const dtgpu_batch &B) {
    FlatRounds r;
    if (B.tier_list[0].empty() || !B.cfg.flat || B.tier_blocks[0] > FLAT_MAX_BLOCKS) return r;
    const size_t lds = size_t(flat_index_bytes(B.tier_blocks[0]));
    const size_t gran = (lds + 1279) / 1280 * 1280;
    r.resident = std::min<size_t>(32, 163840 / std::max<size_t>(gran, 1280)) * size_t(std::max(B.n_cu, 1));
    if (B.cfg.late_from) r.resident = size_t(std::min<uint64_t>(B.cfg.late_from, SIZE_MAX));
    r.order.assign(B.tier_list[0].begin(), B.tier_list[0].end());
    std::stable_sort(r.order.begin(), r.order.end(), [&](uint32_t a, uint32_t b) { return B.n_lv[a] > B.n_lv[b]; });
    return r;
}
template <typename NOps>
std::vector<uint8_t> late_documents(const dtgpu_batch &B, const SegSettings &sc, NOps n_ops) {
    std::vector<uint8_t> late(B.n, 0);
    if (!sc.on || !B.cfg.seg_late) return late;
    const FlatRounds r = flat_rounds(B);
    const size_t resident = r.resident;
    const std::vector<uint32_t> &order = r.order;
    // (a batch of many rounds: its last round's worth, the documents that end the batch)
    const size_t from = std::max(resident, order.size() > resident ? order.size() - resident : size_t(0));
    for (size_t k = from; k < order.size(); k++)
        if (order[k] < B.n && n_ops(order[k]) >= 128) late[order[k]] = 1;
    return late;
}
// The late pipeline's documents (dt_batch.hpp late_pipe): every flat-tier document past the first
// resident round, cut or not, when the tier has fewer than two rounds' worth (a batch of many rounds
// keeps the GPU full with one pipeline: DESIGN §5a found late cutting neutral there) and no other
// LDS tier has documents -- those tiers replay on the side streams the late pipeline runs on, and
// with the split pass on (the default) such a batch is a split pass, which wins: the two are never
// combined.  Empty: no late pipeline.
std::vector<uint8_t> late_pipe_documents(const dtgpu_batch &B) {
    if (!B.cfg.late_pipe) return {};
    for (int t = 1; t < kLdsTiers; t++) if (!B.tier_list[t].empty()) return {};
    const FlatRounds r = flat_rounds(B);
    if (!r.resident || r.order.size() <= r.resident || r.order.size() >= 2 * r.resident) return {};
    std::vector<uint8_t> late(B.n, 0);
    for (size_t k = r.resident; k < r.order.size(); k++) late[r.order[k]] = 1;
    return late;
}
// Per replay document, the document it belongs to: a segment document's document, else itself.
std::vector<uint32_t> segment_owners(const dtgpu_batch &B) {
    std::vector<uint32_t> owner(B.docs.size());
    for (size_t d = 0; d < B.docs.size(); d++) owner[d] = uint32_t(d);
    for (const SegGroup &g : B.seg_groups)
        for (uint32_t k = 1; k < g.count; k++) owner[B.seg_docs[g.first + k]] = B.seg_docs[g.first];
    return owner;
}
// The batch's critical replays (DOC_CRITICAL): a batch whose longest replay unit -- a document
// replayed whole, by the cut planner's cost (SEG_W_OP per op run + LVs); a segment, by its
// document's cost over its segment count -- is at
// least 3x the median gives the units within half of it the top wave priority, as long as they are
// at most an eighth of the units (mixed batches: git-makefile's 50 uncut documents among 1,500
// segments and documents; a batch of equal documents marks none).  DTGPU_CRITICAL=0: off.
void mark_critical(dtgpu_batch &B) {
    for (DocDesc &d : B.docs) d.flags &= ~DOC_CRITICAL;
    if (!B.cfg.critical || B.docs.size() < 2) return;
    std::vector<uint32_t> per(B.docs.size(), 1);   // segments of each unit's document
    for (const SegGroup &g : B.seg_groups)
        for (uint32_t k = 0; k < g.count; k++) per[B.seg_docs[g.first + k]] = g.count;
    const std::vector<uint32_t> owner = segment_owners(B);
    std::vector<double> cost;   // replay units (fast-forwarded documents do not replay)
    std::vector<uint32_t> unit;
    for (size_t i = 0; i < B.docs.size(); i++) {
        if (B.docs[i].flags & DOC_FF) continue;
        const size_t o = owner[i];
        const double runs = o < B.n_runs.size() ? double(B.n_runs[o]) : 0.0;
        cost.push_back((double(SEG_W_OP) * runs + double(B.docs[i].n_lv)) / per[i]);
        unit.push_back(uint32_t(i));
    }
    if (cost.size() < 2) return;
    std::vector<double> srt = cost;
    std::nth_element(srt.begin(), srt.begin() + srt.size() / 2, srt.end());
    const double med = srt[srt.size() / 2], mx = *std::max_element(cost.begin(), cost.end());
    if (mx < 3.0 * med) return;
    size_t n = 0;
    for (double c : cost) n += c >= mx / 2;
    if (8 * n > cost.size()) return;
    for (size_t k = 0; k < cost.size(); k++)
        if (cost[k] >= mx / 2) B.docs[unit[k]].flags |= DOC_CRITICAL;
}
// Blame batches (dt_blame.hpp): after the cut documents' groups, every uncut tracker document
// (tier[i] != -2) becomes a segment group of one -- seg_lo = 0, seg_hi = ~0, seg_u = 0 as
// reset_doc left them, a source list for its inserted characters -- so its replay writes its
// visible items in document order (materialise_src) and the combine step its text.
void add_blame_groups(dtgpu_batch &B, const std::vector<int> &tier, const std::vector<uint64_t> &n_ins, Totals &T) {
    B.n_cut_groups = uint32_t(B.seg_groups.size());
    if (!B.cfg.blame) return;
    for (size_t i = 0; i < B.n; i++) {
        DocDesc &d = B.docs[i];
        if (tier[i] == -2 || d.src_off != ~0ull) continue;
        d.src_off = T.src;
        d.src_cap = uint32_t(n_ins[i]);
        T.src += n_ins[i];
        B.seg_groups.push_back(SegGroup{uint32_t(B.seg_docs.size()), 1});
        B.seg_docs.push_back(uint32_t(i));
    }
}
// The blame kernels' descriptors and scratch, once the arenas and the fast-forward layout exist.
dtgpu_status stage_blame(dtgpu_batch &B, const Totals &T) {
    if (!B.cfg.blame) return DTGPU_OK;
    hipStream_t s = B.stream;
    if (!B.blame) B.blame = std::make_unique<dtgpu_batch::Blame>();
    dtgpu_batch::Blame &M = *B.blame;
    M.docs.assign(B.n, BlameDoc{});
    std::vector<uint32_t> last(B.n, 0xFFFFFFFFu);
    for (const SegGroup &g : B.seg_groups) last[B.seg_docs[g.first]] = B.seg_docs[g.first + g.count - 1];
    uint64_t bits = 0;
    uint32_t n_ff = 0;
    for (size_t i = 0; i < B.n; i++) {
        BlameDoc &q = M.docs[i];
        const DocDesc &d = B.docs[i];
        const bool ff = B.ff_doc[i] != 0;
        const uint32_t ffi = ff ? n_ff++ : 0;   // stage_ff lays the linear documents out in this order
        if (B.host_status[i] != OK) continue;
        q.arun_off = d.arun_off;
        q.n_aruns = d.n_aruns;
        q.n_lv = d.n_lv;
        q.bits_off = bits;
        bits += (uint64_t(d.n_lv) + 31) / 32;
        if (ff) {
            q.kind = BLAME_FF;
            q.last = ffi;
        } else if (last[i] != 0xFFFFFFFFu) {
            q.kind = BLAME_TRACKER;
            q.last = last[i];
            q.src_off = B.docs[last[i]].src_off;
            q.cap = B.docs[last[i]].src_cap;
        }
    }
    DTGPU_CK(M.d_docs.upload(M.docs, s));
    DTGPU_CK(M.d_bits.alloc(std::max<uint64_t>(bits, 1)));
    DTGPU_CK(M.d_len.alloc(std::max<size_t>(B.n, 1)));
    DTGPU_CK(M.d_count.alloc(2 * std::max<size_t>(B.n, 1)));
    DTGPU_CK(hipMemsetAsync(M.d_len.p, 0, std::max<size_t>(B.n, 1) * sizeof(uint32_t), s));
    for (hipEvent_t &e : M.ev) if (!e) DTGPU_CK(hipEventCreate(&e));
    BlameParams &p = M.p;
    p.docs = M.d_docs.p; p.n_docs = uint32_t(B.n);
    p.aruns = B.d_aruns.p; p.src = B.d_src.p; p.results = B.d_results.p;
    p.bits = M.d_bits.p; p.len = M.d_len.p; p.count = M.d_count.p;
    p.ff_docs = B.f_docs.p; p.pa = B.f_pa.p; p.pb = B.f_pb.p; p.ca = B.f_ca.p; p.cb = B.f_cb.p;
    M.stats[3] = 4 * T.src;   // bytes of the source-list arena; the run arena is added when it is sized
    return DTGPU_OK;
}
// The replay's arenas, once every document and segment is laid out (after the upload of the
// document descriptors): the tier lists, the per-LV, block, out and index arenas, the results, and
// the segments' source-list arena and combine step.
dtgpu_status alloc_arenas(dtgpu_batch &B, const Totals &T, const uint32_t *cbyte, const uint8_t *content) {
    hipStream_t s = B.stream;
    DTGPU_CK(B.d_lists.upload(tier_lists(B), s));
    DTGPU_CK(B.d_pos.alloc(T.pc));
    DTGPU_CK(B.d_ao.alloc(T.pc));
    DTGPU_CK(B.d_items.alloc(T.blk * 64));
    DTGPU_CK(B.d_m2.alloc(2 * T.blk));
    DTGPU_CK(B.d_out.alloc(T.out));
    DTGPU_CK(B.d_gidx.alloc(T.gidx));
    DTGPU_CK(B.d_fb.alloc(n_lds_docs(B) + 1));
    DTGPU_CK(B.d_counter.alloc(2));
    DTGPU_CK(B.d_results.alloc(B.docs.size()));
    DTGPU_CK(hipMemsetAsync(B.d_results.p, 0, std::max<size_t>(B.docs.size(), 1) * sizeof(DocResult), s));
    DTGPU_CK(B.d_src.alloc(std::max<uint64_t>(T.src, 1)));
    if (!B.seg_groups.empty()) {
        DTGPU_CK(B.d_groups.upload(B.seg_groups, s));
        DTGPU_CK(B.d_segdocs.upload(B.seg_docs, s));
    }
    CombineParams &c = B.comb;
    c.groups = B.d_groups.p; c.seg_docs = B.d_segdocs.p; c.n_groups = uint32_t(B.seg_groups.size());
    c.docs = B.d_docs.p; c.results = B.d_results.p; c.src = B.d_src.p; c.out = B.d_out.p;
    c.cbyte = cbyte; c.content = content;
    c.n_cu = uint32_t(B.n_cu);
    return DTGPU_OK;
}

// ---- linear histories (dt_ff.hip) ---------------------------------------------------------------
// A document checks out on the fast-forward path when its whole history is one graph entry: the
// reference's merge then fast-forwards through every op (merge.rs:811-840; Graph::push extends
// the last entry whenever a span continues it, so one entry <=> a linear history).
struct FFIn { uint64_t op_off; uint32_t n_ops; uint32_t doc; };   // op runs: quads into `ops`
// The fast-forward layout of the batch's linear documents: segments of FF_RUNS op runs, the
// composition pairs of every level, the copy chunks.  out_off / out_cap / lv_off / content_off /
// ascii come from B.docs (the documents' normal layout); the tracker documents become the
// pass's prep / plan list.
hipError_t stage_ff(dtgpu_batch &B, const std::vector<FFIn> &in, const uint32_t *ops, const uint32_t *cbyte,
                    const uint8_t *content, hipStream_t s) {
    hipError_t e = hipSuccess;
    B.pass_mark = B.cfg.pass_mark;   // (profiling runs: tools/traffic.py)
    std::vector<uint32_t> track;
    for (size_t i = 0; i < B.n; i++)
        if (!B.ff_doc[i]) track.push_back(uint32_t(i));
    B.n_track = uint32_t(track.size());
    B.n_ff = uint32_t(in.size());
    if ((e = B.d_track.upload(track, s)) != hipSuccess) return e;
    B.prep.doc_list = B.d_track.p;
    B.prep.n_docs = B.n_track;
    B.plan.doc_list = B.d_track.p;
    B.plan.n_docs = B.n_track;
    if (in.empty()) return hipSuccess;
    std::vector<FFDoc> docs;
    std::vector<FFSeg> segs;
    std::vector<std::vector<FFPair>> lv;
    std::vector<FFChunk> chunks;
    for (const FFIn &f : in) {
        const DocDesc &d = B.docs[f.doc];
        FFDoc q{};
        q.op_off = f.op_off; q.n_ops = f.n_ops; q.result = f.doc;
        q.lv_off = d.lv_off; q.content_off = d.content_off; q.ascii = d.ascii;
        q.out_off = d.out_off; q.out_cap = d.out_cap;
        q.first_seg = uint32_t(segs.size());
        q.n_seg = (f.n_ops + FF_RUNS - 1) / FF_RUNS;
        q.piece_off = uint64_t(FF_PIECES) * q.first_seg;
        while ((1u << q.levels) < q.n_seg) q.levels++;
        const uint32_t di = uint32_t(docs.size());
        for (uint32_t k = 0; k < q.n_seg; k++)
            segs.push_back(FFSeg{di, k * FF_RUNS, std::min<uint32_t>(FF_RUNS, f.n_ops - k * FF_RUNS), 0});
        if (lv.size() < q.levels) lv.resize(q.levels);
        for (uint32_t k = 0; k < q.levels; k++) {
            const uint32_t g = 1u << k;
            for (uint32_t a = 0; a < q.n_seg; a += 2 * g) lv[k].push_back(FFPair{di, a, a + g < q.n_seg ? a + g : FF_NONE, 0});
        }
        for (uint64_t c = 0; c < d.out_cap; c += FF_CHUNK) chunks.push_back(FFChunk{di, uint32_t(c)});
        docs.push_back(q);
    }
    if (lv.size() > 32) return hipErrorInvalidValue;
    FFParams &p = B.ff;
    p = FFParams{};
    std::vector<FFPair> pairs;
    for (size_t k = 0; k < lv.size(); k++) {
        p.level_off[k] = uint32_t(pairs.size());
        append(pairs, lv[k]);
    }
    p.level_off[lv.size()] = uint32_t(pairs.size());
    const size_t slots = size_t(FF_PIECES) * segs.size();
    if ((e = B.f_docs.upload(docs, s)) != hipSuccess || (e = B.f_segs.upload(segs, s)) != hipSuccess ||
        (e = B.f_pairs.upload(pairs, s)) != hipSuccess || (e = B.f_chunks.upload(chunks, s)) != hipSuccess ||
        (e = B.f_delta.alloc(segs.size())) != hipSuccess || (e = B.f_bad.alloc(docs.size())) != hipSuccess ||
        (e = B.f_pa.alloc(4 * slots)) != hipSuccess || (e = B.f_pb.alloc(4 * slots)) != hipSuccess ||
        (e = B.f_ca.alloc(segs.size())) != hipSuccess || (e = B.f_cb.alloc(segs.size())) != hipSuccess ||
        (e = B.f_boff.alloc(slots)) != hipSuccess)
        return e;
    p.ops = ops; p.cbyte = cbyte; p.content = content;
    p.out = B.d_out.p; p.results = B.d_results.p;
    p.docs = B.f_docs.p; p.segs = B.f_segs.p; p.pairs = B.f_pairs.p; p.chunks = B.f_chunks.p;
    p.n_docs = uint32_t(docs.size()); p.n_segs = uint32_t(segs.size());
    p.n_chunks = uint32_t(chunks.size()); p.n_levels = uint32_t(lv.size());
    p.delta = B.f_delta.p; p.bad = B.f_bad.p; p.boff = B.f_boff.p;
    p.pa = B.f_pa.p; p.pb = B.f_pb.p; p.ca = B.f_ca.p; p.cb = B.f_cb.p;
    return hipSuccess;
}

}  // namespace

// xf: a transformed-ops batch (iter_xf_operations): host plans in TransformedOpsIter order
// (build_xf_plan), every document on the HBM-index tier, never-deleted masks / totals and the
// per-LV transformed-position arena allocated.
dtgpu_status stage(std::vector<Prepared> &prep, const dtgpu_batch_opts *opts, dtgpu_batch **out, bool xf) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return DTGPU_ERR_NO_DEVICE;
    auto B = std::make_unique<dtgpu_batch>();
    B->cfg = settings_for(opts);
    if (xf) B->cfg.blame = false;   // (dtgpu_batch_create_xf refuses the option)
    B->device = opts ? opts->device : 0;
    const size_t n = prep.size();
    if (begin_batch(*B, n) != DTGPU_OK) return DTGPU_ERR_HIP;
    DTGPU_CK(hipStreamCreateWithFlags(&B->stream, hipStreamNonBlocking));
    DTGPU_CK(hipEventCreate(&B->ev0)); DTGPU_CK(hipEventCreate(&B->ev_mid)); DTGPU_CK(hipEventCreate(&B->ev1)); DTGPU_CK(hipEventCreate(&B->ev_prep));
    hipStream_t s = B->stream;
    const int threads = threads_for(opts, n);
    const bool force_host = xf || B->cfg.host_plan;

    // ---- 1. device planner inputs; a sizing pass of the planner gives exact stream sizes ----
    std::vector<PlanDesc> pdesc(n);
    uint64_t erec_words = 0;
    uint32_t lds_entries = 0, max_agents = 0;
    {
        std::vector<uint32_t> par, pent, pch, pcnt, child, tip, aruns, erec, doff, dense, base_rows;
        std::vector<Cmd> opc;
        uint64_t base_total = 0, n_entries = 0;
        for (size_t i = 0; i < n; i++) {
            Prepared &p = prep[i];
            PlanDesc &q = pdesc[i];
            std::memset(&q, 0, sizeof q);
            q.skip = 1;
            if (p.status != OK) continue;
            const PlanInput &pi = p.pi;
            const uint64_t ne = pi.est.size() / 2;
            const bool host = force_host || !pi.device_ok || pi.n_chains > PLAN_MAX_AGENTS ||
                              ne > PLAN_MAX_LDS_ENTRIES || ne * std::max<uint32_t>(pi.n_chains, 1) > (64ull << 20);
            if (host) p.host_plan = true;
            q.skip = host ? 1 : 0;
            q.e_off = n_entries;
            q.par_off = par.size();
            q.child_off = child.size();
            q.op_off = opc.size();
            q.arun_off = aruns.size() / 4;
            q.tip_off = tip.size() / 2;
            q.erec_off = erec.size();
            q.doff_off = doff.size();
            q.dense_off = dense.size();
            q.base_off = base_total;
            q.prow_off = base_total;   // host-staged: the base rows arrive filled (build_plan_input)
            q.row_stride = pi.n_chains;
            q.ne = uint32_t(ne);
            q.n_agents = pi.n_chains;
            q.n_aruns = uint32_t(pi.aruns.size() / 4);
            q.ntip = uint32_t(pi.tip.size() / 2);
            q.n_lv = uint32_t(p.log.n_lv);
            append(aruns, pi.aruns);   // also the replay's tie-break runs
            if (host) continue;
            append(par, pi.par); append(pent, pi.pent); append(pch, pi.pch); append(pcnt, pi.pcnt);
            append(child, pi.child); append(opc, pi.opc);
            append(tip, pi.tip); append(erec, pi.erec); append(doff, pi.doff); append(dense, pi.dense);
            if (pi.prow.size() == ne * pi.n_chains) append(base_rows, pi.prow);
            else base_rows.resize(base_rows.size() + ne * pi.n_chains, 0);
            base_total += ne * pi.n_chains;
            n_entries += ne;
            lds_entries = std::max<uint32_t>(lds_entries, uint32_t(ne));
            max_agents = std::max<uint32_t>(max_agents, pi.n_chains);
        }
        DTGPU_CK(B->p_par.upload(par, s)); DTGPU_CK(B->p_pent.upload(pent, s)); DTGPU_CK(B->p_child.upload(child, s));
        DTGPU_CK(B->p_pch.upload(pch, s)); DTGPU_CK(B->p_pcnt.upload(pcnt, s));
        DTGPU_CK(B->p_opc.upload(opc, s)); DTGPU_CK(B->d_aruns.upload(aruns, s)); DTGPU_CK(B->p_tip.upload(tip, s));
        DTGPU_CK(B->p_erec.upload(erec, s)); DTGPU_CK(B->p_doff.upload(doff, s)); DTGPU_CK(B->p_dense.upload(dense, s));
        DTGPU_CK(B->p_base.upload(base_rows, s));
        erec_words = erec.size();
    }
    B->plan.prow = B->p_base.p;
    std::vector<PlanResult> pres;
    if (size_plans(*B, pdesc, erec_words, lds_entries, max_agents, pres, nullptr) != DTGPU_OK) return DTGPU_ERR_HIP;
    // documents the device planner declined are planned on the host
    std::vector<uint8_t> reason(n, 0);
    for (size_t i = 0; i < n; i++) {
        if (prep[i].status != OK) continue;
        if (pdesc[i].skip) reason[i] = force_host ? 1 : 2;
        else if (pres[i].status != PLAN_OK) { prep[i].host_plan = true; reason[i] = uint8_t(16 + pres[i].status); }
    }
    parallel_for(n, threads, [&](size_t i) {
        Prepared &p = prep[i];
        if (p.status == OK && p.host_plan)
            p.status = xf ? build_xf_plan_from(p.log, p.xf_from, p.xf_merge, p.plan, p.xf_first) : build_plan(p.log, p.plan);
    });

    // ---- 2. per-document layout ---------------------------------------------------------------
    std::vector<Cmd> hcmds;     // host plans, at their documents' offsets
    std::vector<uint32_t> htlist, cbyte;
    std::vector<uint8_t> content;
    Totals T;
    std::vector<int> seg_tier(n, -2);          // replay tier per document (-2: not replayed)
    std::vector<uint64_t> n_ins(n, 0);         // inserted characters per document
    for (size_t i = 0; i < n; i++) {
        Prepared &p = prep[i];
        B->host_status[i] = p.status;
        B->n_lv[i] = p.log.n_lv;
        B->n_runs[i] = p.log.ops.size();
        B->total_lv += p.log.n_lv;
        DocDesc &d = B->docs[i];
        reset_doc(d);
        d.arun_off = pdesc[i].arun_off * 4;
        if (p.status != OK) { pdesc[i].skip = 1; continue; }
        const DocFacts f = facts_of(p.log);
        n_ins[i] = f.n_ins;
        // Host staging checks the block capacity before the fast-forward branch, device staging
        // (stage_device) after it: a linear document past the limit is ErrCapacity here and checks
        // out there.  A known inconsistency, kept as it is.
        if (over_block_limit(f.n_ins)) { B->host_status[i] = ErrCapacity; pdesc[i].skip = 1; continue; }
        if (p.host_plan) {
            B->host_planned[i] = reason[i] ? reason[i] : 2;
            pdesc[i].skip = 1;
            d.cmd_off = T.cmd;
            d.tlist_off = T.tlist;
            d.ncmd = uint32_t(p.plan.cmds.size());
            hcmds.resize(T.cmd);
            htlist.resize(T.tlist);
            append(hcmds, p.plan.cmds);
            append(htlist, p.plan.tlist);
            T.cmd += p.plan.cmds.size();
            T.tlist += p.plan.tlist.size();
        } else {
            plan_slots(*B, d, pdesc[i], pres[i], T);
        }
        describe(d, f);
        d.lv_off = T.lv;
        d.pc_off = T.lv;
        d.content_off = content.size();
        d.n_aruns = uint32_t(p.pi.aruns.size() / 4);
        cbyte.insert(cbyte.end(), p.log.ins_cbyte.begin(), p.log.ins_cbyte.end());
        content.insert(content.end(), p.log.ins_content.begin(), p.log.ins_content.end());
        T.lv += p.log.n_lv;
        if (!xf && B->cfg.ff && f.linear) layout_ff_doc(*B, i, f, T);
        else seg_tier[i] = layout_tracker_doc(*B, i, f, xf, T);
    }
    // host-planned documents' agent runs are not in the planner arrays: append them
    {
        std::vector<uint32_t> extra;
        uint64_t base_q = B->d_aruns.n / 4;
        for (size_t i = 0; i < n; i++) {
            if (!B->host_planned[i]) continue;
            B->docs[i].arun_off = (base_q + extra.size() / 4) * 4;
            append(extra, prep[i].pi.aruns.empty() ? prep[i].plan.agent_runs : prep[i].pi.aruns);
        }
        if (!extra.empty()) {
            std::vector<uint32_t> all(B->d_aruns.n);
            if (B->d_aruns.n)
                DTGPU_CK(hipMemcpyAsync(all.data(), B->d_aruns.p, all.size() * 4, hipMemcpyDeviceToHost, s));
            DTGPU_CK(hipStreamSynchronize(s));
            append(all, extra);
            DevBuf<uint32_t> fresh;
            DTGPU_CK(fresh.upload(all, s));
            std::swap(B->d_aruns.p, fresh.p);
            std::swap(B->d_aruns.n, fresh.n);
            B->plan.aruns = B->d_aruns.p;
        }
    }
    // cut replay: long documents' later LV ranges as documents of their own
    T.pc = T.lv;
    if (!xf) {
        SegSettings sc = seg_settings(B->cfg);
        for (uint32_t i : seg_candidates(n, sc, B->n_cu, B->cfg.seg_fair, [&](size_t k) { return seg_tier[k] != -2 ? prep[k].log.ops.size() : 0; })) {
            SegInput si;
            seg_input_from_log(prep[i].log, si);
            const std::vector<SegCut> cuts = plan_segments(si, sc);
            if (cuts.size() >= 2) add_segments(*B, i, cuts, seg_tier[i], T);
        }
        add_blame_groups(*B, seg_tier, n_ins, T);
    }
    hcmds.resize(T.cmd);
    htlist.resize(T.tlist);
    DTGPU_CK(B->d_cmds.upload(hcmds, s));
    DTGPU_CK(B->d_tlist.upload(htlist, s));
    DTGPU_CK(B->p_docs.upload(pdesc, s));
    B->plan.docs = B->p_docs.p;
    B->plan.cmds = B->d_cmds.p;
    B->plan.tlist = B->d_tlist.p;
    DTGPU_CK(B->d_cbyte.upload(cbyte, s));
    DTGPU_CK(B->d_content.upload(content, s));
    mark_critical(*B);
    DTGPU_CK(B->d_docs.upload(B->docs, s));
    if (alloc_arenas(*B, T, B->d_cbyte.p, B->d_content.p) != DTGPU_OK) return DTGPU_ERR_HIP;
    {   // linear documents: their op runs as the decoder's quads (lv, len, pos, kind | fwd << 1)
        std::vector<FFIn> ffin;
        std::vector<uint32_t> quads;
        for (size_t i = 0; i < n; i++) {
            if (!B->ff_doc[i]) continue;
            ffin.push_back(FFIn{quads.size() / 4, uint32_t(prep[i].log.ops.size()), uint32_t(i)});
            for (const OpRun &r : prep[i].log.ops)
                quads.insert(quads.end(), {uint32_t(r.lv), uint32_t(r.len), uint32_t(r.pos), uint32_t(r.kind) | (uint32_t(r.fwd) << 1)});
        }
        DTGPU_CK(B->f_ops.upload(quads, s));
        DTGPU_CK(stage_ff(*B, ffin, B->f_ops.p, B->d_cbyte.p, B->d_content.p, s));
    }
    if (stage_blame(*B, T) != DTGPU_OK) return DTGPU_ERR_HIP;
    if (B->blame) {   // the agent ids' names, as the agent_names export lays them out
        B->blame->names.resize(n);
        for (size_t i = 0; i < n; i++)
            for (const std::string &nm : prep[i].log.agent_names) {
                B->blame->names[i].push_back(uint8_t(nm.size()));
                B->blame->names[i].insert(B->blame->names[i].end(), nm.begin(), nm.end());
            }
    }
    if (xf) {
        DTGPU_CK(B->d_mup.alloc(T.blk));
        DTGPU_CK(B->d_tup.alloc(T.blk + 2 * n));
        DTGPU_CK(B->d_xf.alloc(T.lv));
    }
    DTGPU_CK(hipStreamSynchronize(s));
    B->xf_mode = xf;
    if (set_tier_params(*B, B->d_cbyte.p, B->d_content.p) != DTGPU_OK) return DTGPU_ERR_HIP;
    *out = B.release();
    return DTGPU_OK;
}

// Device-staged batch: `.dt` bytes -> device decode -> device prep -> planner sizing pass ->
// replay layout.  The host only reads back per-document counts to size the arenas.  Documents
// the device path hands back (decoder or prep limits) get status DTGPU_DECODE_DEFER.
// `dec` is a decoded handle (dtgpu_decode_create: decoded here; dtgpu_decode_add: already merged).
//
// xf: the merge form (dtgpu_decode_xf_from).  Every document is the projected history of a merge
// request; plan_kernel_xf plans it from the request's `from`, and every document replays on the
// HBM tier in transformed-ops mode: no fast-forward layout, no segments, no split or late pipeline.
dtgpu_status stage_device(dtgpu_decoded *dec, const dtgpu_batch_opts *opts, dtgpu_batch **out, XfStage *xf) {
    auto B = std::make_unique<dtgpu_batch>();
    B->cfg = settings_for(opts);
    if (xf) B->cfg.blame = false;
    B->device = dec->device;
    B->dec.reset(dec);
    dtgpu_decoded &Dd = *B->dec;
    const size_t n = Dd.n;
    if (begin_batch(*B, n) != DTGPU_OK) return DTGPU_ERR_HIP;
    B->stream = Dd.stream;   // one stream for decode, prep, plan and replay
    Dd.stream = nullptr;     // owned by the batch from here on
    DTGPU_CK(hipEventCreate(&B->ev0)); DTGPU_CK(hipEventCreate(&B->ev_mid)); DTGPU_CK(hipEventCreate(&B->ev1));
    DTGPU_CK(hipEventCreate(&B->ev_dec)); DTGPU_CK(hipEventCreate(&B->ev_prep));
    DTGPU_CK(hipEventCreateWithFlags(&B->ev_w0, hipEventDisableTiming));
    DTGPU_CK(hipEventCreateWithFlags(&B->ev_w1, hipEventDisableTiming));
    hipStream_t s = B->stream;
    if (!Dd.merged) {
        if (launch_decode(Dd.P, s)) return DTGPU_ERR_HIP;
        DTGPU_CK(hipMemcpyAsync(Dd.res.data(), Dd.d_res.p, n * sizeof(DecodeResult), hipMemcpyDeviceToHost, s));
        DTGPU_CK(hipStreamSynchronize(s));
    }
    stage_prof("stage: decode pass");

    // ---- prep layout ----------------------------------------------------------------------------
    std::vector<PrepDesc> pd(n);
    uint64_t o_par = 0, o_op = 0, o_arun = 0, o_tip = 0, o_erec = 0, o_doff = 0, o_dense = 0, o_rows = 0, o_scr = 0;
    uint32_t max_e = 1;
    for (size_t i = 0; i < n; i++) {
        const DecodeResult &r = Dd.res[i];
        const DecodeDesc &d = Dd.desc[i];
        PrepDesc &q = pd[i];
        std::memset(&q, 0, sizeof q);
        q.skip = 1;
        uint32_t st = r.status;
        if (st == OK && !r.content_complete) st = ErrCheckout;   // content.unwrap() in apply_to
        if (st == OK && (r.n_lv >= MAX_PLAN_LV || r.n_entries > PLAN_MAX_LDS_ENTRIES)) st = DECODE_DEFER;
        if (st == OK && xf && xf->skip[i]) st = DECODE_DEFER;   // answered by the caller
        B->host_status[i] = st;
        B->n_lv[i] = r.n_lv;
        B->n_runs[i] = r.n_ops;
        if (st != OK) continue;
        q.skip = 0;
        q.d_op = d.op_off; q.d_arun = d.arun_off; q.d_ent = d.ent_off; q.d_poff = d.poff_off; q.d_par = d.par_off;
        q.d_ver = d.ver_off; q.d_agent = d.agent_off; q.d_in = d.in_off;
        q.n_ops = r.n_ops; q.n_aruns = r.n_aruns; q.ne = r.n_entries; q.n_par = r.n_parents; q.n_ver = r.n_version;
        q.n_agents = r.n_agents; q.n_lv = uint32_t(r.n_lv);
        q.o_par = o_par; o_par += r.n_parents;
        q.o_child = q.o_par;
        q.o_op = o_op; o_op += r.n_ops;
        q.o_arun = o_arun; o_arun += r.n_aruns;
        q.o_tip = o_tip; o_tip += r.n_version;
        q.o_erec = o_erec; o_erec += uint64_t(EREC_WORDS) * r.n_entries;
        q.o_doff = o_doff; o_doff += PREP_MAX_CHAINS + 1;
        q.o_dense = o_dense; o_dense += r.n_lv;
        q.o_rows = o_rows; o_rows += uint64_t(PREP_MAX_CHAINS) * r.n_entries;
        q.row_stride = PREP_MAX_CHAINS;
        q.o_scr = o_scr; o_scr += prep_scratch_words(r.n_parents, r.n_entries);
        max_e = std::max<uint32_t>(max_e, r.n_entries);
    }
    DTGPU_CK(B->p_par.alloc(o_par)); DTGPU_CK(B->p_pent.alloc(o_par)); DTGPU_CK(B->p_pch.alloc(o_par)); DTGPU_CK(B->p_pcnt.alloc(o_par));
    DTGPU_CK(B->p_child.alloc(o_par)); DTGPU_CK(B->p_opc.alloc(o_op)); DTGPU_CK(B->d_aruns.alloc(4 * o_arun));
    DTGPU_CK(B->p_tip.alloc(2 * o_tip)); DTGPU_CK(B->p_erec.alloc(o_erec)); DTGPU_CK(B->p_doff.alloc(o_doff));
    DTGPU_CK(B->p_dense.alloc(o_dense)); DTGPU_CK(B->pr_rows.alloc(o_rows)); DTGPU_CK(B->pr_scr.alloc(o_scr));
    // prep stores each entry's parent vector at the chains that exist by then; the words past
    // them stay zero from here on (every pass writes the same words)
    DTGPU_CK(hipMemsetAsync(B->pr_rows.p, 0, std::max<uint64_t>(o_rows, 1) * sizeof(uint32_t), s));
    DTGPU_CK(B->pr_docs.upload(pd, s)); DTGPU_CK(B->pr_res.alloc(n));
    PrepParams &pp = B->prep;
    pp.in = Dd.in.p;
    pp.d_ops = Dd.ops.p; pp.d_aruns = Dd.aruns.p; pp.d_ent = Dd.ent.p; pp.d_poff = Dd.poff.p; pp.d_par = Dd.par.p;
    pp.d_ver = Dd.ver.p; pp.d_agents = Dd.agents.p;
    pp.par = B->p_par.p; pp.pent = B->p_pent.p; pp.pch = B->p_pch.p; pp.pcnt = B->p_pcnt.p; pp.child = B->p_child.p;
    pp.aruns = B->d_aruns.p; pp.tip = B->p_tip.p; pp.erec = B->p_erec.p; pp.doff = B->p_doff.p; pp.dense = B->p_dense.p;
    pp.rows = B->pr_rows.p; pp.scr = B->pr_scr.p; pp.opc = B->p_opc.p;
    if (B->cfg.prep_chains) {
        DTGPU_CK(B->pr_chain.alloc(std::max<size_t>(n, 1)));
        pp.chain_flag = B->pr_chain.p;
    }
    pp.docs = B->pr_docs.p; pp.results = B->pr_res.p; pp.n_docs = uint32_t(n); pp.max_entries = max_e;
    // debug mode (DTGPU_DEBUG, or DTGPU_PREP_CHECK alone): the bounds-checked prep kernel
    pp.check = B->cfg.prep_check ? 1u : 0u;
    if (launch_prep(pp, s)) return DTGPU_ERR_HIP;
    std::vector<PrepResult> prr(n);
    DTGPU_CK(hipMemcpyAsync(prr.data(), B->pr_res.p, n * sizeof(PrepResult), hipMemcpyDeviceToHost, s));
    DTGPU_CK(hipStreamSynchronize(s));
    stage_prof("stage: prep layout + pass");

    // ---- planner sizing pass ----------------------------------------------------------------------
    std::vector<PlanDesc> pdesc(n);
    uint64_t base_total = 0;
    uint32_t lds_entries = 0, max_agents = 0;
    for (size_t i = 0; i < n; i++) {
        PlanDesc &q = pdesc[i];
        std::memset(&q, 0, sizeof q);
        q.skip = 1;
        if (B->host_status[i] != OK) continue;
        if (prr[i].status != PREP_OK) { B->host_status[i] = prr[i].status == PREP_WIDE ? DECODE_DEFER : ErrCheckout; continue; }
        const PrepDesc &r = pd[i];
        q.skip = 0;
        q.par_off = r.o_par; q.child_off = r.o_child; q.op_off = r.o_op; q.arun_off = r.o_arun; q.tip_off = r.o_tip;
        q.erec_off = r.o_erec; q.doff_off = r.o_doff; q.dense_off = r.o_dense;
        q.base_off = base_total;
        q.prow_off = r.o_rows;   // device-staged: the prep kernel's parent vectors
        q.coff_off = r.o_scr + prep_kids_offset(r.n_par, r.ne);   // walk kernel: children per entry
        q.poff_off = r.d_poff;
        q.row_stride = PREP_MAX_CHAINS;
        q.ne = r.ne; q.n_agents = prr[i].n_chains; q.n_aruns = r.n_aruns; q.ntip = r.n_ver; q.n_lv = r.n_lv;
        if (xf) { q.xf_off = xf->from_off[i]; q.n_from = uint32_t(xf->from_off[i + 1] - xf->from_off[i]); }
        base_total += uint64_t(r.ne) * std::max<uint32_t>(prr[i].n_chains, 1);
        lds_entries = std::max<uint32_t>(lds_entries, r.ne);
        max_agents = std::max<uint32_t>(max_agents, prr[i].n_chains);
    }
    DTGPU_CK(B->p_base.alloc(base_total));
    PlanParams &q = B->plan;
    q.prow = B->pr_rows.p;
    q.coff = B->pr_scr.p;
    q.poff = Dd.poff.p;
    if (xf) { q.xf = 1; q.xf_from = xf->d_from; }
    std::vector<PlanResult> pres;
    std::vector<uint32_t> wres;
    if (size_plans(*B, pdesc, o_erec, lds_entries, max_agents, pres, &wres) != DTGPU_OK) return DTGPU_ERR_HIP;
    // the walks of every later pass are the same walks: their stacks get the deepest one seen
    // here (plus slack), not PLAN_TODO_CAP -- the walk kernel's LDS then leaves room for the
    // chain decomposition's waves beside it.  (A deeper walk would fail its document visibly,
    // PLAN_TODO_FULL; the walk is deterministic, so none does.)
    if (!xf) {
        uint32_t deep = 0;
        for (size_t i = 0; i < n; i++)
            if (!pdesc[i].skip && pres[i].status == PLAN_OK) deep = std::max(deep, wres[2 * i] >> 16);
        q.todo_cap = std::min<uint32_t>(PLAN_TODO_CAP, (deep + 16 + 1) & ~1u);
    }

    stage_prof("stage: planner sizing pass");
    // ---- replay layout ---------------------------------------------------------------------------
    Totals T;
    std::vector<int> seg_tier(n, -2);          // replay tier per document (-2: not replayed)
    std::vector<uint64_t> n_ins(n, 0);         // inserted characters per document
    for (size_t i = 0; i < n; i++) {
        DocDesc &d = B->docs[i];
        reset_doc(d);
        if (B->host_status[i] != OK) { pdesc[i].skip = 1; continue; }
        if (pres[i].status != PLAN_OK) { B->host_status[i] = DECODE_DEFER; pdesc[i].skip = 1; continue; }
        const DecodeResult &r = Dd.res[i];
        const DecodeDesc &dd = Dd.desc[i];
        const DocFacts f = facts_of(r, prr[i]);
        n_ins[i] = f.n_ins;
        plan_slots(*B, d, pdesc[i], pres[i], T);
        if (xf) { xf->xf_first[i] = pres[i].xf_first; xf->n_xf[i] = pres[i].n_xf; }
        describe(d, f);
        d.lv_off = dd.lv_off;                 // per-LV arenas share the decoder's LV numbering
        d.pc_off = dd.lv_off;
        d.content_off = dd.content_off;       // inserted text read in place
        d.arun_off = pd[i].o_arun * 4;
        d.n_aruns = r.n_aruns;
        if (!xf && B->cfg.ff && f.linear) {
            layout_ff_doc(*B, i, f, T);
            B->total_lv += r.n_lv;
            continue;
        }
        // Device staging checks the block capacity inside the tracker branch, host staging (stage)
        // before the fast-forward branch: a linear document past the limit checks out here and is
        // ErrCapacity there.  A known inconsistency, kept as it is.
        if (over_block_limit(f.n_ins)) { B->host_status[i] = ErrCapacity; pdesc[i].skip = 1; continue; }
        B->total_lv += r.n_lv;
        seg_tier[i] = layout_tracker_doc(*B, i, f, xf != nullptr, T);
    }
    T.lv = Dd.cbyte.n;
    // cut replay: long documents' later LV ranges as documents of their own
    T.pc = T.lv;
    if (!xf) {
        SegSettings sc = seg_settings(B->cfg);
        const std::vector<uint32_t> cand = seg_candidates(n, sc, B->n_cu, B->cfg.seg_fair, [&](size_t k) { return seg_tier[k] != -2 ? Dd.res[k].n_ops : 0u; });
        std::vector<uint8_t> late = late_documents(*B, sc, [&](size_t k) { return Dd.res[k].n_ops; });
        for (uint32_t i : cand) late[i] = 0;
        std::vector<uint32_t> all = cand;
        for (size_t i = 0; i < n; i++) if (late[i]) all.push_back(uint32_t(i));
        std::sort(all.begin(), all.end());
        B->late_doc = late_pipe_documents(*B);
        B->late_pipe = !B->late_doc.empty();
        // the cut planning itself (cut_kernel in sizing mode), one launch over every candidate
        // and one copy back: the same deterministic kernel every pass then runs against the
        // arenas reserved here (a host plan would need each document's decoded arrays back)
        std::vector<SegGroup> sg;
        std::vector<SegPlan> sp;
        std::vector<uint32_t> sdocs;
        uint64_t sscr = 0;
        uint32_t smax_ne = 0;
        for (uint32_t i : all) {
            const DecodeResult &r = Dd.res[i];
            SegSettings c = sc;
            if (late[i]) { c.max_seg = 2; c.ops_per_seg = std::max<uint64_t>(1, r.n_ops / 2); }
            const uint32_t S = uint32_t(std::min<uint64_t>(c.max_seg, r.n_ops / c.ops_per_seg));
            if (S < 2 || r.n_entries == 0 || r.n_lv >= 0x7FFFFFFFull || r.n_entries > PLAN_MAX_LDS_ENTRIES) continue;
            sg.push_back(SegGroup{uint32_t(sdocs.size()), S});
            sdocs.push_back(i);
            sp.push_back(SegPlan{c.w_op, S, sscr});
            sscr += (cut_scratch_words(r.n_entries) + 1) & ~1ull;
            smax_ne = std::max<uint32_t>(smax_ne, r.n_entries);
        }
        std::vector<uint32_t> sized(sg.size() * CUT_SIZED_WORDS);
        if (!sg.empty()) {
            DevBuf<SegGroup> dg;
            DevBuf<SegPlan> dp;
            DevBuf<uint32_t> dd, dscr, dout;
            DTGPU_CK(dg.upload(sg, s)); DTGPU_CK(dp.upload(sp, s)); DTGPU_CK(dd.upload(sdocs, s));
            DTGPU_CK(dscr.alloc(std::max<uint64_t>(sscr, 1))); DTGPU_CK(dout.alloc(sized.size()));
            CutParams c{};
            c.d_ops = Dd.ops.p; c.d_ent = Dd.ent.p; c.d_poff = Dd.poff.p; c.d_par = Dd.par.p;
            c.pdocs = B->pr_docs.p;
            c.groups = dg.p; c.seg_docs = dd.p; c.plans = dp.p;
            c.scr = dscr.p;
            c.n_groups = uint32_t(sg.size());
            c.max_ne = smax_ne;
            c.sized = dout.p;
            if (launch_cut(c, s)) return DTGPU_ERR_HIP;
            DTGPU_CK(hipMemcpyAsync(sized.data(), dout.p, sized.size() * 4, hipMemcpyDeviceToHost, s));
            DTGPU_CK(hipStreamSynchronize(s));
        }
        uint64_t scr = 0;
        for (size_t g = 0; g < sg.size(); g++) {
            const uint32_t i = sdocs[g];
            const uint32_t *z = sized.data() + g * CUT_SIZED_WORDS;
            std::vector<SegCut> cuts(std::min<uint32_t>(z[0], 64));
            for (size_t k = 0; k < cuts.size(); k++) cuts[k] = SegCut{z[1 + 4 * k], z[2 + 4 * k], z[3 + 4 * k], z[4 + 4 * k]};
            if (cuts.size() < 2 || !add_segments(*B, i, cuts, seg_tier[i], T)) continue;
            B->seg_plans.push_back(SegPlan{sp[g].w_op, sp[g].n_targets, scr});
            for (const SegCut &k : cuts) B->seg_caps.push_back(SegCap{k.u, uint32_t(k.ins), k.lo, k.hi});
            scr += (cut_scratch_words(Dd.res[i].n_entries) + 1) & ~1ull;
            B->cut.max_ne = std::max<uint32_t>(B->cut.max_ne, Dd.res[i].n_entries);
        }
        DTGPU_CK(B->d_cutscr.alloc(std::max<uint64_t>(scr, 1)));
        add_blame_groups(*B, seg_tier, n_ins, T);
    }
    stage_prof("stage: layout + cut plans");
    // every later pass: parent-vector rows as wide as the document's chains (staging counted
    // them), four-word aligned for the planner's 16-byte row loads -- a 64-word row per entry
    // spread two live words over a cache line of their own (prep's stores, the planner's loads)
    uint32_t widest = 0;
    for (size_t i = 0; i < n; i++) {
        if (pd[i].skip || prr[i].status != PREP_OK) continue;
        const uint32_t rs = std::min<uint32_t>((std::max<uint32_t>(prr[i].n_chains, 1) + 3) & ~3u, PREP_MAX_CHAINS);
        pd[i].row_stride = rs;
        pdesc[i].row_stride = rs;
        widest = std::max(widest, rs);
    }
    B->prep.chain_w = widest;   // the chain decomposition's LDS ring rows, as wide as needed
    DTGPU_CK(B->pr_docs.upload(pd, s));
    B->prep.docs = B->pr_docs.p;
    DTGPU_CK(B->d_cmds.alloc(T.cmd));
    DTGPU_CK(B->d_tlist.alloc(T.tlist));
    DTGPU_CK(B->p_docs.upload(pdesc, s));
    B->plan.docs = B->p_docs.p;
    B->plan.cmds = B->d_cmds.p;
    B->plan.tlist = B->d_tlist.p;
    {   // every segment's LV range is the pass's cut planning's to write (poisoned here: a replay
        // without it fails, ErrCheckout site 30)
        mark_critical(*B);
        std::vector<DocDesc> up = B->docs;
        for (uint32_t g = 0; g < B->n_cut_groups; g++)
            for (uint32_t k = 0; k < B->seg_groups[g].count; k++) {
                DocDesc &e = up[B->seg_docs[B->seg_groups[g].first + k]];
                e.seg_lo = 0xFFFFFFFFu; e.seg_hi = 0;
            }
        DTGPU_CK(B->d_docs.upload(up, s));
    }
    if (alloc_arenas(*B, T, Dd.cbyte.p, Dd.content.p) != DTGPU_OK) return DTGPU_ERR_HIP;
    {   // linear documents: the fast-forward layout over the decoder's op runs, in place
        std::vector<FFIn> ffin;
        for (size_t i = 0; i < n; i++)
            if (B->ff_doc[i]) ffin.push_back(FFIn{Dd.desc[i].op_off, Dd.res[i].n_ops, uint32_t(i)});
        DTGPU_CK(stage_ff(*B, ffin, Dd.ops.p, Dd.cbyte.p, Dd.content.p, s));
    }
    if (stage_blame(*B, T) != DTGPU_OK) return DTGPU_ERR_HIP;
    if (B->n_cut_groups) {
        DTGPU_CK(B->d_plans.upload(B->seg_plans, s));
        DTGPU_CK(B->d_caps.upload(B->seg_caps, s));
        CutParams &c = B->cut;
        c.d_ops = Dd.ops.p; c.d_ent = Dd.ent.p; c.d_poff = Dd.poff.p; c.d_par = Dd.par.p;
        c.pdocs = B->pr_docs.p;
        c.groups = B->d_groups.p;
        c.seg_docs = B->d_segdocs.p;
        c.plans = B->d_plans.p;
        c.caps = B->d_caps.p;
        c.docs = B->d_docs.p;
        c.scr = B->d_cutscr.p;
        c.pent = B->p_pent.p;
        c.n_groups = B->n_cut_groups;
        if (!B->ev_cut) DTGPU_CK(hipEventCreateWithFlags(&B->ev_cut, hipEventDisableTiming));
    }
    if (xf) {   // the transformed-ops replay's arenas, as stage() allocates them for its xf batches
        DTGPU_CK(B->d_mup.alloc(T.blk));
        DTGPU_CK(B->d_tup.alloc(T.blk + 2 * n));
        DTGPU_CK(B->d_xf.alloc(T.lv));
        B->xf_mode = true;
    }
    DTGPU_CK(hipStreamSynchronize(s));
    stage_prof("stage: arenas + uploads");
    if (set_tier_params(*B, Dd.cbyte.p, Dd.content.p) != DTGPU_OK) return DTGPU_ERR_HIP;
    B->wstream = B->side[kSideStreams - 1];   // the smallest side tier's stream (see wstream)
    // split pass: when an LDS tier rides a side stream and other documents exist, its
    // documents' prep and plan do not wait for everyone else's (a skewed batch's longest replays
    // start as soon as their own plans are done).  The tier: the critical documents' (DOC_CRITICAL,
    // the batch's longest replays), else the biggest non-empty one.  Its segment documents'
    // documents are planned there too (the main pipeline's replay waits for those plans).
    if (B->cfg.split && !xf) {
        int tb = -1;
        for (int t = kLdsTiers - 1; t >= 1 && tb < 0; t--)
            for (uint32_t d : B->tier_list[t])
                if (B->docs[d].flags & DOC_CRITICAL) { tb = t; break; }
        for (int t = kLdsTiers - 1; t >= 1 && tb < 0; t--)
            if (!B->tier_list[t].empty()) tb = t;
        if (tb >= 1) {
            const std::vector<uint32_t> owner = segment_owners(*B);
            std::vector<uint8_t> big(n, 0);
            std::vector<uint32_t> lst;   // in the tier's order
            for (uint32_t d : B->tier_list[tb])
                if (owner[d] < n && !big[owner[d]]) { big[owner[d]] = 1; lst.push_back(owner[d]); }
            const size_t nb = lst.size();
            for (size_t i = 0; i < n; i++)
                if (!big[i] && !B->ff_doc[i]) lst.push_back(uint32_t(i));
            if (lst.size() > nb) {
                DTGPU_CK(B->d_split.upload(lst, s));
                DTGPU_CK(hipStreamSynchronize(s));
                B->split = true;
                B->split_tier = tb;
                if (!B->ws_side) DTGPU_CK(hipStreamCreateWithFlags(&B->ws_side, hipStreamNonBlocking));
                if (!B->ev_sw0) DTGPU_CK(hipEventCreateWithFlags(&B->ev_sw0, hipEventDisableTiming));
                if (!B->ev_sw1) DTGPU_CK(hipEventCreateWithFlags(&B->ev_sw1, hipEventDisableTiming));
                B->n_big = uint32_t(nb);
                B->n_rest = uint32_t(lst.size() - nb);
            }
        }
    }
    // late pipeline: the prep / plan lists of its two pipelines.  A split pass wins (it already
    // runs a side pipeline on these streams; late_pipe_documents leaves no batch to both).
    if (B->split) B->late_pipe = false;
    if (B->late_pipe) {
        std::vector<uint32_t> lst, late;
        for (size_t i = 0; i < n; i++)
            if (!B->ff_doc[i]) (B->late_doc[i] ? late : lst).push_back(uint32_t(i));
        B->n_first = uint32_t(lst.size());
        B->n_late = uint32_t(late.size());
        append(lst, late);
        DTGPU_CK(B->d_late.upload(lst, s));
        DTGPU_CK(hipStreamSynchronize(s));
        if (!B->ev_sw0) DTGPU_CK(hipEventCreateWithFlags(&B->ev_sw0, hipEventDisableTiming));
        if (!B->ev_sw1) DTGPU_CK(hipEventCreateWithFlags(&B->ev_sw1, hipEventDisableTiming));
        if (!B->ev_lprep) DTGPU_CK(hipEventCreateWithFlags(&B->ev_lprep, hipEventDisableTiming));
        if (!B->ev_lgo) DTGPU_CK(hipEventCreateWithFlags(&B->ev_lgo, hipEventDisableTiming));
    }
    stage_prof("stage: split setup");
    *out = B.release();
    return DTGPU_OK;
}

}  // namespace dtgpu
