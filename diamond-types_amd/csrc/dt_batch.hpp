// dt_batch.hpp -- what the batch code shares (internal): the batch settings, struct dtgpu_batch,
// and the staging entry points.  dtgpu_stage.cpp lays a batch out in HBM, dtgpu_pass.cpp runs
// checkout passes over it and reads results back, dtgpu_api.cpp holds the oplog ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <thread>
#include <vector>

#include "../../include/dtgpu.h"
#include "dt_blame.hpp"
#include "dt_cut.hpp"
#include "dt_decoded.hpp"
#include "dt_devbuf.hpp"
#include "dt_device.hpp"
#include "dt_encoder.hpp"
#include "dt_ff.hpp"
#include "dt_host.hpp"
#include "dt_prep.hpp"

namespace dtgpu {

// Checkouts replay on the per-item tracker (dt_replay.hip); its LDS tiers go by index bytes: a
// document whose expected index fits a tier replays with its index in LDS, friendsforever-sized
// documents many per CU, a node_nodecc-sized one alone on a CU.  Bigger documents and LDS
// overflows replay on the HBM-index tier.
constexpr int kLdsTiers = kMaxLdsTiers;

// How a batch checks out: the defaults, then dtgpu_batch_opts (the API's knobs), then the DTGPU_*
// environment overrides (experiments, A/B runs, tests), read once when the batch is created.
struct Settings {
    bool ff = true;            // linear histories on the fast-forward path (dt_ff.hip)
    bool seg = true;           // cut replay (long documents as LV segments on several waves)
    uint64_t seg_ops = 500;    // op runs per segment (raised to the batch's fair share per wave slot)
    uint32_t seg_max = 32;     // segments per document: measured against 16-64 on the six cut traces
    uint32_t seg_w = SEG_W_OP; // the cut planner's cost weight of an op run
    bool seg_fair = true;      // the fair-share floor on seg_ops
    bool seg_late = true;      // late documents of the smallest tier cut once
    bool late_pipe = true;     // ... and prepared, planned and replayed in a pipeline of their own
    uint64_t late_from = 0;    // the flat tier's resident round in documents (0: from the device; tests)
    // expected inserted chars per block when sizing a document's LDS index: blocks end up ~43
    // items full on the benchmark traces (cut_point, dt_replay.hip), sized at 40 (tests force the
    // LDS overflow -> HBM tier hand-back with a large value)
    uint64_t lds_fill = 40;
    bool flat = true;          // the smallest LDS tier on the flat 2-level index (IX_FLAT)
    bool prep_chains = true;   // prep as three launches, the chain decomposition four documents per wave
    bool walk_overlap = true;  // the walk on its own stream beside prep's second half
    bool host_plan = false;    // walk plans built on the host
    bool split = true;         // split pass for skewed batches
    bool critical = true;      // critical replays first, at top wave priority
    bool fallback = true;      // LDS-tier documents that outgrow their index replay on the HBM tier
    bool prio = true;          // late workgroups of the flat tier raise their wave priority
    uint32_t tog_waves = 0;    // 1: retreat / advance passes on one wave (else DTGPU_TOG_WAVES helpers)
    uint32_t tog_mw_lds = 32 * 1024;   // LDS index bytes from which a tier gets helper waves
    uint32_t debug = 0;        // bit 0 invariant checks, bit 1 cycle profile (the instrumented kernels)
    bool prep_check = false;   // the bounds-checked prep kernel
    bool pass_mark = false;    // every pass opens with pass_mark_kernel (tools/traffic.py)
    bool plan_prof = false, enc_prof = false;
    bool blame = false;        // the batch also produces each document's blame (dt_blame.hpp): every uncut
                               // tracker document a segment group of one, no late cuts, no late pipeline
    uint32_t enc_lds_text = 0;
};
Settings settings_for(const dtgpu_batch_opts *o);

// Per-document replay layout: block capacity, HBM index bytes, LDS tier.
struct Layout { uint32_t max_blocks; uint64_t gidx; int tier; uint32_t tier_blocks; };

// A document on its way into a host-staged batch: the decoded oplog and the planner's inputs.
struct Prepared {
    Status status = OK;
    HostOpLog log;
    PlanInput pi;
    Plan plan;             // host plan: only for documents the device planner declines
    bool host_plan = false;
    std::vector<uint64_t> xf_from, xf_merge;   // transformed-ops batches: the merge to report
    size_t xf_first = 0;                       // first reported command of the plan
};

inline int threads_for(const dtgpu_batch_opts *opts, size_t n) {
    int t = opts && opts->host_threads > 0 ? opts->host_threads : int(std::thread::hardware_concurrency());
    if (t < 1) t = 1;
    if (size_t(t) > n) t = int(std::max<size_t>(n, 1));
    return t;
}
template <typename F>
void parallel_for(size_t n, int threads, F f) {
    std::atomic<size_t> next{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++)
        pool.emplace_back([&] { for (size_t i; (i = next.fetch_add(1)) < n;) f(i); });
    for (auto &th : pool) th.join();
}

}  // namespace dtgpu

struct dtgpu_batch {
    int device = 0;
    int n_cu = 256;
    dtgpu::Settings cfg;   // opts + DTGPU_* overrides, fixed at creation
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev_mid = nullptr, ev1 = nullptr;
    size_t n = 0;
    std::vector<uint32_t> host_status;   // decode / plan status per doc
    std::vector<uint64_t> n_lv;
    std::vector<dtgpu::DocDesc> docs;
    std::vector<uint32_t> tier_list[dtgpu::kLdsTiers], large_list;   // LDS tiers (index bytes), HBM tier
    std::vector<uint8_t> host_planned;   // 0: device-planned; else why the host planned it
    uint32_t tier_blocks[dtgpu::kLdsTiers] = {};
    uint32_t debug = 0;
    hipStream_t side[dtgpu::kSideStreams] = {};   // big LDS tiers run beside the small ones, one stream each
    hipEvent_t ev_fork = nullptr, ev_join[dtgpu::kSideStreams] = {};
    // device-staged split pass: the biggest LDS tier's documents run prep -> plan -> replay on
    // that tier's side stream, beside the other documents' prep and plan (d_split: the big
    // tier's documents, then the rest)
    bool split = false;
    int split_tier = -1;
    uint32_t n_big = 0, n_rest = 0;
    DevBuf<uint32_t> d_split;
    // device-staged late pipeline (Settings::late_pipe): the flat tier's documents past its first
    // resident round run prep -> plan -> replay on side[0] (their walk on side[1]), so that the
    // first round's replay starts without them (dtgpu_pass.cpp launch_late_pass).  d_late: the
    // first round's documents and every document outside
    // the flat tier (n_first), then the late ones (n_late), laid out as d_split; the flat tier's
    // replay list holds the first round's workgroups (flat_first), then the late documents'.
    // Never with a split pass.
    bool late_pipe = false;
    std::vector<uint8_t> late_doc;   // per document: 1 = in the late pipeline (empty: no late set)
    uint32_t n_first = 0, n_late = 0, flat_first = 0;
    DevBuf<uint32_t> d_late;
    hipEvent_t ev_lprep = nullptr, ev_lgo = nullptr;   // the late prep is done; the late plan may start
    uint64_t alg_in_bytes = 0, total_lv = 0;
    float last_plan_ms = 0, last_replay_ms = 0;

    // device planner inputs (the decoded oplogs) and scratch
    DevBuf<uint32_t> p_par, p_pent, p_pch, p_pcnt, p_child, p_tip, p_erec, p_doff, p_dense;
    DevBuf<dtgpu::Cmd> p_opc;
    DevBuf<uint32_t> p_base;
    DevBuf<uint32_t> p_order;    // two-phase planner: each document's walk order (by entry arena offset)
    DevBuf<uint32_t> p_walk;     // walk_kernel: per document {status, steps}
    DevBuf<uint32_t> pr_chain;   // prep's three-launch pass: per document its stage (dt_prep.hpp)
    DevBuf<dtgpu::PlanDesc> p_docs;
    DevBuf<dtgpu::PlanResult> p_results;
    dtgpu::PlanParams plan{};
    uint32_t n_gpu_planned = 0;

    DevBuf<dtgpu::Cmd> d_cmds;
    DevBuf<uint32_t> d_tlist, d_cbyte, d_aruns, d_pos, d_items, d_lists, d_counter;
    DevBuf<unsigned long long> d_ao, d_m2, d_mup;
    DevBuf<uint32_t> d_tup, d_xf;   // transformed-ops batches only
    bool xf_mode = false;
    DevBuf<uint8_t> d_content, d_out, d_gidx;
    DevBuf<uint32_t> d_fb;   // [0] = count, then the handed-back documents
    DevBuf<dtgpu::DocDesc> d_docs;
    DevBuf<dtgpu::DocResult> d_results;
    dtgpu::BatchParams tier[dtgpu::kLdsTiers]{}, large{};
    // cut replay: segment documents (docs[n..]: a long document's later LV ranges, replayed
    // beside its first one) and the combine step that joins their source lists into its text
    std::vector<uint64_t> seg_cost;
    std::vector<uint64_t> first_cost;   // per document: its first segment's LVs when cut (else 0)
    std::vector<uint64_t> n_runs;       // per document: its op runs (mark_critical)
    std::vector<dtgpu::SegGroup> seg_groups;
    std::vector<uint32_t> seg_docs;
    DevBuf<dtgpu::SegGroup> d_groups;
    DevBuf<uint32_t> d_segdocs, d_src;
    dtgpu::CombineParams comb{};
    // device-staged batches: the cut planning runs in every pass (cut_kernel, dt_prep.hpp); staging
    // only reserves each segment's arenas and uploads its descriptor with a poisoned LV range
    std::vector<dtgpu::SegPlan> seg_plans;
    std::vector<dtgpu::SegCap> seg_caps;
    DevBuf<dtgpu::SegPlan> d_plans;
    DevBuf<dtgpu::SegCap> d_caps;
    DevBuf<uint32_t> d_cutscr;
    dtgpu::CutParams cut{};
    hipEvent_t ev_cut = nullptr;
    hipEvent_t ev_splan = nullptr;   // split pass: the big tier's plans are done (segments may
                                     // replay in another tier, on the main stream)

    // device-staged batches (dtgpu_batch_create_device): the decoded oplogs stay in the
    // decoder's arenas (content and per-LV offsets are read there by the replay) and the
    // planner inputs are built by the prep kernel
    std::unique_ptr<dtgpu_decoded> dec;
    DevBuf<uint32_t> pr_rows, pr_scr;
    DevBuf<dtgpu::PrepDesc> pr_docs;
    DevBuf<dtgpu::PrepResult> pr_res;
    dtgpu::PrepParams prep{};
    hipEvent_t ev_dec = nullptr, ev_prep = nullptr;
    // the planner's walk beside prep's second half: a side stream (idle until the replay), since
    // a process gets GPU_MAX_HW_QUEUES = 4 hardware queues and a fifth stream would share one --
    // serialising two replay tiers that should run side by side
    hipStream_t wstream = nullptr;
    hipEvent_t ev_w0 = nullptr, ev_w1 = nullptr;
    hipStream_t ws_side = nullptr;                    // split pass: the side pipeline's walk
    hipEvent_t ev_sw0 = nullptr, ev_sw1 = nullptr;
    float last_decode_ms = 0, last_prep_ms = 0;

    // linear histories (dt_ff.hip): a document whose history is one graph entry checks out on the
    // fast-forward piece table instead of prep -> plan -> replay (staging still prepares and plans
    // it, for the batched encoder); the pass's prep / plan lists hold the other documents
    std::vector<uint8_t> ff_doc;          // per document: 1 = fast-forward path
    uint32_t n_ff = 0, n_track = 0;       // documents on each path
    DevBuf<uint32_t> d_track;             // the tracker's documents (prep / plan doc_list)
    DevBuf<uint32_t> f_ops;               // host-staged batches: op runs as the decoder's quads
    DevBuf<dtgpu::FFDoc> f_docs;
    DevBuf<dtgpu::FFSeg> f_segs;
    DevBuf<dtgpu::FFPair> f_pairs;
    DevBuf<dtgpu::FFChunk> f_chunks;
    DevBuf<int32_t> f_delta;
    DevBuf<uint32_t> f_bad, f_pa, f_pb, f_ca, f_cb, f_boff;
    dtgpu::FFParams ff{};
    bool pass_mark = false;   // DTGPU_PASS_MARK at staging: every pass opens with pass_mark_kernel

    // blame batches (DTGPU_OPT_BLAME, dt_blame.hpp): seg_groups holds the cut groups (n_cut_groups,
    // what the device cut planning plans), then the uncut tracker documents' groups of one.  Every
    // pass counts the runs; the first blame read after it sizes the run arena from the counts,
    // emits the runs and copies them and the documents' statuses back (Blame::h_*).
    uint32_t n_cut_groups = 0;
    struct Blame {
        std::vector<dtgpu::BlameDoc> docs;
        DevBuf<dtgpu::BlameDoc> d_docs;
        DevBuf<uint32_t> d_bits, d_len, d_count;
        DevBuf<uint64_t> d_off;
        DevBuf<dtgpu::BlameRun> d_runs;
        dtgpu::BlameParams p{};
        std::vector<std::vector<uint8_t>> names;   // host-staged: per document, the agent_names export
        hipEvent_t ev[4] = {};                     // around the counting kernels, around the emit
        uint64_t pass = 0, read = 0;               // passes launched; the pass the host copies are of
        std::vector<uint32_t> h_count, h_status;
        std::vector<uint64_t> h_off;
        std::vector<dtgpu::BlameRun> h_runs;
        uint64_t stats[4] = {};
        ~Blame() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    };
    std::unique_ptr<Blame> blame;

    // batched encoder (dtgpu_batch_encode): per-document descriptors, scratch, output
    std::vector<dtgpu::EncDesc> e_desc;
    std::vector<dtgpu::EncResult> e_res;
    DevBuf<dtgpu::EncDesc> e_docs;
    DevBuf<dtgpu::EncResult> e_dres;
    DevBuf<uint32_t> e_w;
    DevBuf<uint8_t> e_b, e_out;
    dtgpu::EncParams enc{};

    ~dtgpu_batch() {
        for (hipEvent_t e : {ev_lprep, ev_lgo, ev_splan, ev_cut, ev_sw0, ev_sw1, ev_w0, ev_w1, ev_dec, ev_prep, ev0, ev_mid, ev1, ev_fork})
            if (e) (void)hipEventDestroy(e);
        if (ws_side) (void)hipStreamDestroy(ws_side);
        for (int k = 0; k < dtgpu::kSideStreams; k++) {
            if (ev_join[k]) (void)hipEventDestroy(ev_join[k]);
            if (side[k]) (void)hipStreamDestroy(side[k]);
        }
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace dtgpu {

// Host-staged batch: decoded oplogs -> uploaded planner arrays -> planner sizing pass -> replay
// layout.  xf: a transformed-ops batch (iter_xf_operations).
dtgpu_status stage(std::vector<Prepared> &prep, const dtgpu_batch_opts *opts, dtgpu_batch **out, bool xf = false);
// Device-staged batch over a decoded handle, which the batch consumes.  xf: the merge form
// (dt_merge.hpp), the handle's documents being the requests' projected histories.
struct XfStage;
dtgpu_status stage_device(dtgpu_decoded *dec, const dtgpu_batch_opts *opts, dtgpu_batch **out, XfStage *xf = nullptr);

}  // namespace dtgpu
