// dtgpu_pass.cpp -- checkout passes over a staged batch (dtgpu_stage.cpp): what one pass enqueues,
// the dtgpu_batch_run* entry points, the batched encoder, and the batch's read-back accessors.
#include <cstdio>
#include <cstring>

#include "dt_batch.hpp"
#include "dt_merge.hpp"

using namespace dtgpu;

namespace {

// Every record / wait between a pass's streams is in this file (DESIGN.md §5e draws each pass
// shape); the launch_* functions only put a kernel on the stream they are given.
int wait_for(hipStream_t s, hipEvent_t e) { return hipStreamWaitEvent(s, e, 0) == hipSuccess ? OK : ErrHip; }
// `to` waits, through e, for what `from` holds so far.
int hop(hipEvent_t e, hipStream_t from, hipStream_t to) {
    return hipEventRecord(e, from) == hipSuccess ? wait_for(to, e) : ErrHip;
}

// Prep then plan for a device-staged batch, as one pipeline: its documents (doc_list / n_docs of
// prep and plan), its cut groups, its stream, its walk stream and the events between the two (w0:
// prep's first half is done).  A whole pass has one pipeline over B's own parameters, a split or
// late-pipeline pass two.  With the three-launch prep and the walk kernel, the walk (CSR mode: it
// needs only prep's first half) runs on the walk stream beside the chain decomposition and prep's
// second half, and the plan kernel waits for it; the pipeline's cut planning (if it has cut groups)
// follows the walk there.
struct Pipe {
    PrepParams prep;
    PlanParams plan;
    CutParams cut;
    hipStream_t s, w;
    hipEvent_t w0, w1, cut_done;
};
Pipe whole_pipe(const dtgpu_batch *B, hipStream_t s) {
    return Pipe{B->prep, B->plan, B->cut, s, B->wstream, B->ev_w0, B->ev_w1, B->ev_cut};
}
// One of a pass's two pipelines: n documents of `list` on s, the walk on w.  It plans no cuts:
// the pass does, once for both.
Pipe list_pipe(const dtgpu_batch *B, hipStream_t s, const uint32_t *list, uint32_t n, hipStream_t w, hipEvent_t w0,
               hipEvent_t w1) {
    Pipe p = whole_pipe(B, s);
    p.prep.doc_list = p.plan.doc_list = list;
    p.prep.n_docs = p.plan.n_docs = n;
    p.cut.n_groups = 0;
    p.w = w; p.w0 = w0; p.w1 = w1; p.cut_done = nullptr;
    return p;
}
bool walk_beside(const dtgpu_batch *B, const Pipe &p) {
    return B->dec && B->n_gpu_planned && p.prep.chain_flag && !p.prep.check && p.plan.coff && p.w &&
           B->cfg.walk_overlap;
}
// The prep half; `mid` (nullable) is recorded at its end on s.
int pipe_prep(dtgpu_batch *B, const Pipe &p, hipEvent_t mid) {
    hipStream_t s = p.s;
    if (!walk_beside(B, p)) {
        if (B->dec && launch_prep(p.prep, s)) return ErrHip;
        if (p.w0 && hipEventRecord(p.w0, s) != hipSuccess) return ErrHip;
        if (launch_cut(p.cut, s)) return ErrHip;   // (after prep: it reads the parents' entries)
        return mid && hipEventRecord(mid, s) != hipSuccess ? ErrHip : OK;
    }
    // the walk reads prep's CSR and the planner only the entry records' heads
    PrepParams pp = p.prep;
    pp.short_rec = 1;
    if (launch_prep_stage(pp, s, 1) || hop(p.w0, s, p.w)) return ErrHip;
    if (launch_walk(p.plan, p.w, true) != OK) return ErrHip;
    if (hipEventRecord(p.w1, p.w) != hipSuccess) return ErrHip;
    // the cut planning after the walk (it reads prep's parent entries), beside prep's second half
    // and the planner (only the replay needs it)
    if (p.cut.n_groups && (launch_cut(p.cut, p.w) || hipEventRecord(p.cut_done, p.w) != hipSuccess))
        return ErrHip;
    if (launch_prep_stage(pp, s, 2) || launch_prep_stage(pp, s, 3)) return ErrHip;
    return mid && hipEventRecord(mid, s) != hipSuccess ? ErrHip : OK;
}
// The plan half: after it, s may replay the pipeline's documents.
int pipe_plan(dtgpu_batch *B, const Pipe &p) {
    hipStream_t s = p.s;
    const bool beside = walk_beside(B, p);
    if (beside && wait_for(s, p.w1)) return ErrHip;
    if (B->n_gpu_planned && launch_plan(p.plan, s, !beside) != OK) return ErrHip;
    if (beside && p.cut.n_groups && wait_for(s, p.cut_done)) return ErrHip;
    return OK;
}
int prep_and_plan(dtgpu_batch *B, const Pipe &p, hipEvent_t mid) {
    const int e = pipe_prep(B, p, mid);
    return e ? e : pipe_plan(B, p);
}

// The instrumented replay kernels (invariant checks, cycle profiles): B->debug is the debug word
// of every tier and of the HBM tier (set_tier_params).
bool instrumented(const dtgpu_batch *B) { return (B->debug & 3u) != 0; }
// LDS tier t >= 1 replays on a side stream of its own, the biggest tier on side[0].
int side_of(int t) { return kLdsTiers - 1 - t; }
// The hand-back counter to zero, on s: one for the batch, every LDS tier appends to it.
int reset_handback(dtgpu_batch *B, hipStream_t s) {
    uint32_t *n = const_cast<uint32_t *>(B->tier[0].fb_count);
    return !n || hipMemsetAsync(n, 0, sizeof(uint32_t), s) == hipSuccess ? OK : ErrHip;
}
// The tail of every tracker pass on s: the HBM tier (its own documents and whatever the LDS tiers
// handed back), then the cut documents' texts joined from their segments'.
int replay_hbm_and_combine(dtgpu_batch *B, hipStream_t s) {
    int e = launch_replay_hbm(B->large, s, instrumented(B));
    // a blame batch: the final lists' lengths, before the combine step rewrites the results of
    // the groups of one
    if (!e && B->blame) e = launch_blame_len(B->blame->p, s);
    return e ? e : launch_combine(B->comb, s);
}
// The replay of a whole pass, or the main pipeline's of a split pass (skip_tier: replayed by the
// side pipeline, which reset the counter).  If an LDS tier has documents: fork from s to every
// side stream, the biggest tiers first, each on its side stream, the smallest on s, and every
// side stream joined back into s -- the split tier's too, with the side pipeline on it.
int replay_all(dtgpu_batch *B, hipStream_t s, int skip_tier = -1) {
    const bool split = skip_tier >= 0;
    // split pass: a segment of a big-tier document may sit in a tier replayed from s
    if (split && !B->seg_groups.empty() && wait_for(s, B->ev_splan)) return ErrHip;
    uint32_t n_lds = 0;
    for (int t = 0; t < kLdsTiers; t++) n_lds += t != skip_tier ? B->tier[t].n_list : 0;
    if (n_lds) {
        if (!split && reset_handback(B, s)) return ErrHip;
        if (hipEventRecord(B->ev_fork, s) != hipSuccess) return ErrHip;
        for (int k = 0; k < kSideStreams; k++)
            if (wait_for(B->side[k], B->ev_fork)) return ErrHip;
        for (int t = kLdsTiers - 1; t >= 0; t--) {
            if (t == skip_tier) continue;
            if (const int e = launch_replay_lds(B->tier[t], t ? B->side[side_of(t)] : s, instrumented(B))) return e;
        }
        for (int k = 0; k < kSideStreams; k++)
            if (hop(B->ev_join[k], B->side[k], s)) return ErrHip;
    } else if (split) {
        // nothing forked, so nothing else joins the side pipeline: it must be done before the
        // HBM tier reads the hand-back queue and before anything synchronising on s sees the
        // batch as finished
        const int k = side_of(skip_tier);
        if (hop(B->ev_join[k], B->side[k], s)) return ErrHip;
    }
    return replay_hbm_and_combine(B, s);
}

// A split pass plans its cuts beside the side pipeline's prep, before the main pipeline's: the cut
// kernel then finds each parent's entry itself.
CutParams cut_before_prep(const dtgpu_batch *B) {
    CutParams c = B->cut;
    c.pent = nullptr;
    return c;
}
// The split pass's side pipeline (see stage_device): after a fork from s, the big tier's prep,
// plan and replay on its side stream.  The hand-back counter is reset first, on s, since both
// pipelines' LDS tiers append to it; the main pipeline's replay_all(skip_tier) joins the side
// stream before the HBM tier.
int launch_split_side(dtgpu_batch *B, hipStream_t s) {
    hipStream_t sb = B->side[side_of(B->split_tier)];
    if (reset_handback(B, s) || hop(B->ev_fork, s, sb)) return ErrHip;
    Pipe p = list_pipe(B, sb, B->d_split.p, B->n_big, B->ws_side, B->ev_sw0, B->ev_sw1);
    if (!walk_beside(B, p)) p.w0 = nullptr;   // (no walk stream in use: nothing waits for prep's first half)
    if (const int e = prep_and_plan(B, p, nullptr)) return e;
    if (hipEventRecord(B->ev_splan, sb) != hipSuccess) return ErrHip;
    // the cut planning on s, beside the side pipeline's prep and plan (the main pipeline's prep
    // follows it there); the side replay waits for it
    if (B->cut.n_groups && (launch_cut(cut_before_prep(B), s) || hop(B->ev_cut, s, sb))) return ErrHip;
    return launch_replay_lds(B->tier[B->split_tier], sb, instrumented(B));
}
// The main pipeline of a split pass: the documents outside the big tier, all on s.
Pipe split_main_pipe(const dtgpu_batch *B, hipStream_t s) {
    return list_pipe(B, s, B->d_split.p + B->n_big, B->n_rest, nullptr, nullptr, nullptr);
}

// The linear documents' checkout (dt_ff.hip) on s: first in a pass, or, in a split pass, right
// after the side pipeline's fork (beside it, before the main pipeline's prep).
int launch_ff_pass(dtgpu_batch *B, hipStream_t s) { return B->n_ff ? launch_ff(B->ff, s) : OK; }
// The tracker part of a pass (prep -> plan -> replay), unless every document fast-forwards.
bool tracker_pass(const dtgpu_batch *B) { return B->n_track != 0 || B->ff_doc.empty(); }

// The events a timed pass records on s between its steps (all null: an untimed pass): at its
// start, when the main pipeline's prep is enqueued, and when its plan is.
struct PassMarks { hipEvent_t start = nullptr, prepped = nullptr, planned = nullptr; };
int mark(hipEvent_t e, hipStream_t s) { return !e || hipEventRecord(e, s) == hipSuccess ? OK : ErrHip; }

// `count` workgroups of the flat tier's list from `first` on, on s.
int replay_flat_range(dtgpu_batch *B, hipStream_t s, uint32_t first, uint32_t count, bool all_late) {
    BatchParams q = B->tier[0];
    q.doc_list += first;
    q.n_list = count;
    q.all_late = all_late ? 1u : 0u;
    return launch_replay_lds(q, s, instrumented(B));
}
// A pass with the late pipeline (dt_batch.hpp late_pipe).  On s: prep and plan of the first
// round's documents, then their replay.  On side[0] (the walk on side[1]), from the end of the
// main pipeline's prep first half on -- the two first halves share no round: the late
// documents' prep, beside the main pipeline's prep and plan.  The cut planning of both sets in
// one launch, where a whole pass has it: on the main pipeline's walk stream after its walk,
// beside the main plan (measured: on the late streams it waits for slots for 3 ms and holds up
// the late chain decomposition, or, after the first round's replay, the late replay).  The first
// round's replay fills every wave slot of the device and its whole documents are the pass's
// critical path, so it must not find a slot taken: s waits for the late prep and the cuts
// (nothing else is in flight then), and the late plan opens one event hop (over the walk stream)
// after the first round's replay is launched -- it and the late replay, every workgroup at the
// raised priority, then queue for the slots the first round frees.  s joins side[0] before the
// HBM tier (its own documents and whatever either launch handed back) and the combine step.
// The hand-back counter is reset once, at the start.  The marks are the main pipeline's, as in
// a split pass.
int launch_late_pass(dtgpu_batch *B, hipStream_t s, const PassMarks &m) {
    hipStream_t sl = B->side[0], w = B->wstream;
    if (reset_handback(B, s)) return ErrHip;
    const Pipe a = list_pipe(B, s, B->d_late.p, B->n_first, w, B->ev_w0, B->ev_w1);
    const Pipe b = list_pipe(B, sl, B->d_late.p + B->n_first, B->n_late, B->side[1], B->ev_sw0, B->ev_sw1);
    int e = pipe_prep(B, a, m.prepped);
    if (e) return e;
    if (wait_for(sl, B->ev_w0) || (e = pipe_prep(B, b, nullptr))) return e ? e : ErrHip;
    if (walk_beside(B, b) && wait_for(sl, b.w1)) return ErrHip;
    if (hipEventRecord(B->ev_lprep, sl) != hipSuccess) return ErrHip;
    if (B->cut.n_groups) {   // (it reads both first halves' parent entries)
        if (wait_for(w, B->ev_w0) || wait_for(w, B->ev_sw0) || launch_cut(B->cut, w) || hipEventRecord(B->ev_cut, w) != hipSuccess)
            return ErrHip;
    }
    if ((e = pipe_plan(B, a)) || (e = mark(m.planned, s))) return e;
    if (wait_for(s, B->ev_lprep) || (B->cut.n_groups && wait_for(s, B->ev_cut))) return ErrHip;
    // (ev_fork: the first round's replay is launched)
    if (hipEventRecord(B->ev_fork, s) != hipSuccess) return ErrHip;
    if ((e = replay_flat_range(B, s, 0, B->flat_first, false))) return e;
    if (wait_for(w, B->ev_fork) || hop(B->ev_lgo, w, sl)) return ErrHip;
    if ((e = pipe_plan(B, b))) return e;
    if ((e = replay_flat_range(B, sl, B->flat_first, B->tier[0].n_list - B->flat_first, true))) return e;
    if (hop(B->ev_join[0], sl, s)) return ErrHip;
    return replay_hbm_and_combine(B, s);
}
// The tracker part of a pass on s, after the fast-forward pass: prep (device-staged: the walker
// inputs first), plan, replay -- every entry point's, timed or not.
int launch_tracker(dtgpu_batch *B, hipStream_t s, const PassMarks &m) {
    if (B->late_pipe) return launch_late_pass(B, s, m);
    int e = prep_and_plan(B, whole_pipe(B, s), m.prepped);
    if (e || (e = mark(m.planned, s))) return e;
    return replay_all(B, s);
}

// One checkout pass on stream s: the pass mark, the split pass's side pipeline, the fast-forward
// pass, prep (device-staged batches; split: the rest's prep), plan, replay.
int launch_pass(dtgpu_batch *B, hipStream_t s, const PassMarks &m = {}) {
    if (B->pass_mark && launch_pass_mark(s)) return ErrHip;
    if (mark(m.start, s)) return ErrHip;
    if (B->xf_mode) {   // every document on the HBM tier; host plans (n_gpu_planned is 0), or a merge
                        // batch (device-staged): prep, then plan_kernel_xf
        if (B->dec && launch_prep(B->prep, s)) return ErrHip;
        if (mark(m.prepped, s)) return ErrHip;
        if (B->n_gpu_planned && launch_plan(B->plan, s) != OK) return ErrHip;
        return mark(m.planned, s) ? ErrHip : launch_replay_xf(B->large, s);
    }
    int e = B->split ? launch_split_side(B, s) : OK;   // (it plans the cuts too)
    if (e) return e;
    // a batch of only linear documents reports their pass as its replay time
    const bool track = tracker_pass(B);
    if (!track && (mark(m.prepped, s) || mark(m.planned, s))) return ErrHip;
    e = launch_ff_pass(B, s);
    if (e || !track) return e;
    if (!B->split) return launch_tracker(B, s, m);
    // prep / plan times are the main pipeline's
    if ((e = prep_and_plan(B, split_main_pipe(B, s), m.prepped)) || (e = mark(m.planned, s))) return e;
    return replay_all(B, s, B->split_tier);
}

// A blame batch's pass ends with the boundary bitmaps and the run counts (dt_blame.hip), on s
// after everything else of the pass; the runs themselves are emitted by the first blame read.
int launch_blame_pass(dtgpu_batch *B, hipStream_t s) {
    if (!B->blame) return OK;
    dtgpu_batch::Blame &M = *B->blame;
    if (hipEventRecord(M.ev[0], s) != hipSuccess || launch_blame_count(M.p, s) || hipEventRecord(M.ev[1], s) != hipSuccess)
        return ErrHip;
    M.pass++;
    return OK;
}
// The runs of the last pass on the host: the counts read back, the run arena sized from them,
// the emit kernel, and one copy of the runs and the documents' statuses.
dtgpu_status read_blame(const dtgpu_batch *B) {
    dtgpu_batch::Blame &M = *B->blame;
    if (M.read == M.pass && M.pass) return DTGPU_OK;
    if (!M.pass) return DTGPU_ERR_ARG;   // no pass has run
    if (hipSetDevice(B->device) != hipSuccess) return DTGPU_ERR_HIP;
    hipStream_t s = B->stream;
    const size_t n = B->n;
    M.h_count.assign(2 * std::max<size_t>(n, 1), 0);
    std::vector<DocResult> dr(n);
    DTGPU_CK(hipStreamSynchronize(s));
    DTGPU_CK(hipEventSynchronize(M.ev[1]));   // (a pass on the caller's stream)
    if (n) {
        DTGPU_CK(hipMemcpyAsync(M.h_count.data(), M.d_count.p, 2 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        DTGPU_CK(hipMemcpyAsync(dr.data(), B->d_results.p, n * sizeof(DocResult), hipMemcpyDeviceToHost, s));
    }
    DTGPU_CK(hipStreamSynchronize(s));
    M.h_off.assign(n + 1, 0);
    M.h_status.assign(n, 0);
    uint64_t chars = 0;
    for (size_t i = 0; i < n; i++) {
        M.h_status[i] = B->host_status[i] != OK ? B->host_status[i] : dr[i].status;
        if (M.h_status[i] != OK) M.h_count[i] = M.h_count[n + i] = 0;
        M.h_off[i + 1] = M.h_off[i] + M.h_count[i];
        chars += M.h_count[n + i];
    }
    const uint64_t total = M.h_off[n];
    if (!M.d_runs.p || M.d_runs.n < total) DTGPU_CK(M.d_runs.alloc(total));   // (a batch of empty texts: one slot)
    if (!M.d_off.p || M.d_off.n < n + 1) DTGPU_CK(M.d_off.alloc(n + 1));
    DTGPU_CK(hipMemcpyAsync(M.d_off.p, M.h_off.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    DTGPU_CK(hipMemsetAsync(M.d_runs.p, 0, std::max<uint64_t>(total, 1) * sizeof(BlameRun), s));
    BlameParams p = M.p;
    p.run_off = M.d_off.p;
    p.runs = M.d_runs.p;
    DTGPU_CK(hipEventRecord(M.ev[2], s));
    if (total && launch_blame_emit(p, s)) return DTGPU_ERR_HIP;
    DTGPU_CK(hipEventRecord(M.ev[3], s));
    M.h_runs.assign(total, BlameRun{});
    if (total) DTGPU_CK(hipMemcpyAsync(M.h_runs.data(), M.d_runs.p, total * sizeof(BlameRun), hipMemcpyDeviceToHost, s));
    DTGPU_CK(hipStreamSynchronize(s));
    float t0 = 0, t1 = 0;
    DTGPU_CK(hipEventElapsedTime(&t0, M.ev[0], M.ev[1]));
    DTGPU_CK(hipEventElapsedTime(&t1, M.ev[2], M.ev[3]));
    M.stats[0] = total;
    M.stats[1] = chars;
    M.stats[2] = uint64_t((t0 + t1) * 1000.0f + 0.5f);
    M.stats[3] = 4 * uint64_t(B->d_src.n) + sizeof(BlameRun) * uint64_t(M.d_runs.n);
    M.read = M.pass;
    return DTGPU_OK;
}

}  // namespace

extern "C" {

dtgpu_status dtgpu_batch_blame(const dtgpu_batch *B, size_t i, dtgpu_blame_run *runs, size_t cap, size_t *n_out) {
    if (!B || !B->blame || i >= B->n) return DTGPU_ERR_ARG;
    if (B->host_status[i] != OK) { if (n_out) *n_out = 0; return dtgpu_status(B->host_status[i]); }
    if (const dtgpu_status st = read_blame(B)) return st;
    const dtgpu_batch::Blame &M = *B->blame;
    if (n_out) *n_out = M.h_status[i] == OK ? M.h_count[i] : 0;
    if (M.h_status[i] != OK) return dtgpu_status(M.h_status[i]);
    if (!runs) return DTGPU_OK;
    if (cap < M.h_count[i]) return DTGPU_ERR_ARG;
    static_assert(sizeof(dtgpu_blame_run) == sizeof(BlameRun), "one layout");
    if (M.h_count[i]) std::memcpy(runs, M.h_runs.data() + M.h_off[i], M.h_count[i] * sizeof(BlameRun));
    return DTGPU_OK;
}
dtgpu_status dtgpu_batch_blame_agents(const dtgpu_batch *B, size_t i, uint8_t *names, size_t cap, size_t *n_out) {
    if (!B || !B->blame || i >= B->n) return DTGPU_ERR_ARG;
    if (B->host_status[i] != OK) { if (n_out) *n_out = 0; return dtgpu_status(B->host_status[i]); }
    size_t n = 0;
    if (B->dec) {   // device-staged: the decoder's agent table
        if (hipSetDevice(B->device) != hipSuccess) return DTGPU_ERR_HIP;
        n = dtgpu_decode_export(B->dec.get(), i, DTGPU_EXPORT_AGENT_NAMES, nullptr, 0);
        if (n_out) *n_out = n;
        if (!names) return DTGPU_OK;
        if (cap < n) return DTGPU_ERR_ARG;
        return dtgpu_decode_export(B->dec.get(), i, DTGPU_EXPORT_AGENT_NAMES, names, cap) == n ? DTGPU_OK : DTGPU_ERR_HIP;
    }
    const std::vector<uint8_t> &blob = B->blame->names[i];
    n = blob.size();
    if (n_out) *n_out = n;
    if (!names) return DTGPU_OK;
    if (cap < n) return DTGPU_ERR_ARG;
    if (n) std::memcpy(names, blob.data(), n);
    return DTGPU_OK;
}
dtgpu_status dtgpu_batch_blame_stats(const dtgpu_batch *B, uint64_t out[4]) {
    if (!B || !B->blame || !out) return DTGPU_ERR_ARG;
    if (const dtgpu_status st = read_blame(B)) return st;
    for (int k = 0; k < 4; k++) out[k] = B->blame->stats[k];
    return DTGPU_OK;
}

dtgpu_status dtgpu_batch_xf_positions(dtgpu_batch *B, size_t i, uint32_t *out, size_t cap, size_t *n_out) {
    if (!B || i >= B->n || !B->xf_mode) return DTGPU_ERR_ARG;
    if (B->host_status[i] != OK) return dtgpu_status(B->host_status[i]);
    const size_t n = size_t(B->n_lv[i]);
    if (n_out) *n_out = n;
    if (!out) return DTGPU_OK;
    if (cap < n) return DTGPU_ERR_ARG;
    DocResult r;
    if (hipMemcpyAsync(&r, B->d_results.p + i, sizeof r, hipMemcpyDeviceToHost, B->stream) != hipSuccess ||
        (n && hipMemcpyAsync(out, B->d_xf.p + B->docs[i].lv_off, n * 4, hipMemcpyDeviceToHost, B->stream) != hipSuccess) ||
        hipStreamSynchronize(B->stream) != hipSuccess)
        return DTGPU_ERR_HIP;
    return r.status == OK ? DTGPU_OK : dtgpu_status(r.status);
}
dtgpu_status dtgpu_batch_run_e2e_timed(dtgpu_batch *B, float ms[4]) {
    if (!B || !B->dec || B->dec->merged) return DTGPU_ERR_ARG;
    if (hipSetDevice(B->device) != hipSuccess) return DTGPU_ERR_HIP;
    hipStream_t s = B->stream;
    // decode + prep + plan + replay from the `.dt` bytes in HBM
    if (hipEventRecord(B->ev_dec, s) != hipSuccess) return DTGPU_ERR_HIP;
    if (launch_decode(B->dec->P, s)) return DTGPU_ERR_HIP;
    if (hipEventRecord(B->ev_prep, s) != hipSuccess) return DTGPU_ERR_HIP;
    if (launch_ff_pass(B, s)) return DTGPU_ERR_HIP;   // linear documents (dt_ff.hip)
    // (the same tracker pass as dtgpu_batch_run's, its marks between prep, plan and replay; not
    // through launch_pass: no pass mark, and a split-eligible batch runs as one whole pipeline)
    const int st = tracker_pass(B) ? launch_tracker(B, s, PassMarks{nullptr, B->ev0, B->ev_mid})
                                   : (mark(B->ev0, s) || mark(B->ev_mid, s) ? ErrHip : OK);
    if (st) return dtgpu_status(st);
    if (launch_blame_pass(B, s)) return DTGPU_ERR_HIP;
    if (hipEventRecord(B->ev1, s) != hipSuccess) return DTGPU_ERR_HIP;
    if (hipEventSynchronize(B->ev1) != hipSuccess) return DTGPU_ERR_HIP;
    float td = 0, tp = 0, tl = 0, tr = 0;
    if (hipEventElapsedTime(&td, B->ev_dec, B->ev_prep) != hipSuccess || hipEventElapsedTime(&tp, B->ev_prep, B->ev0) != hipSuccess ||
        hipEventElapsedTime(&tl, B->ev0, B->ev_mid) != hipSuccess || hipEventElapsedTime(&tr, B->ev_mid, B->ev1) != hipSuccess)
        return DTGPU_ERR_HIP;
    B->last_decode_ms = td; B->last_prep_ms = tp; B->last_plan_ms = tl; B->last_replay_ms = tr;
    if (ms) { ms[0] = td; ms[1] = tp; ms[2] = tl; ms[3] = tr; }
    return DTGPU_OK;
}
dtgpu_status dtgpu_batch_encode(dtgpu_batch *B, uint32_t flags, float *kernel_ms) {
    if (!B || !B->dec || B->xf_mode) return DTGPU_ERR_ARG;
    if (flags & ~uint32_t(DTGPU_ENCODE_FULL)) return DTGPU_ERR_ARG;
    if (hipSetDevice(B->device) != hipSuccess) return DTGPU_ERR_HIP;
    hipStream_t s = B->stream;
    if (B->e_desc.empty() && B->n) {   // layout once per batch
        const dtgpu_decoded &Dd = *B->dec;
        B->e_desc.assign(B->n, EncDesc{});
        uint64_t w = 0, b = 0, o = 0;
        uint32_t max_agents = 1, max_text = 0;
        for (size_t i = 0; i < B->n; i++) {
            EncDesc &e = B->e_desc[i];
            e.skip = 1;
            if (B->host_status[i] != OK) continue;
            const DecodeResult &r = Dd.res[i];
            const DecodeDesc &d = Dd.desc[i];
            const DocDesc &dd = B->docs[i];
            e.skip = 0;
            e.in_off = d.in_off; e.arun_off = d.arun_off; e.ent_off = d.ent_off; e.poff_off = d.poff_off;
            e.par_off = d.par_off; e.content_off = d.content_off; e.lv_off = d.lv_off; e.agent_off = d.agent_off;
            e.cmd_off = dd.cmd_off;
            e.ncmd = dd.ncmd; e.n_aruns = r.n_aruns; e.ne = r.n_entries; e.n_agents = r.n_agents;
            e.n_lv = uint32_t(r.n_lv); e.n_content = r.n_content;
            e.doc_id_off = r.doc_id_off; e.doc_id_len = r.doc_id_len;
            e.w_off = w; w += enc_words(e.ne, e.ncmd, e.n_aruns, e.n_agents);
            e.b_off = b; b += (r.n_content + lz4_bound(r.n_content) + 15) / 16 * 16;   // 16-B aligned text
            // output bound: header + names + doc id + every stream at its widest varints
            const uint64_t cap = 128 + 11ull * r.n_agents + 64 + (r.doc_id_len != 0xFFFFFFFFu ? r.doc_id_len : 0) +
                                 30ull * (uint64_t(r.n_aruns) + r.n_entries) + 20ull * e.ncmd + 10ull * r.n_entries +
                                 10ull * r.n_parents + lz4_bound(r.n_content) + d.in_len;   // names are in the input
            e.out_off = o; e.out_cap = uint32_t(std::min<uint64_t>(cap, 0xFFFFFFF0ull)); o += (e.out_cap + 15) / 16 * 16;   // 16-B aligned (CRC reads)
            max_agents = std::max(max_agents, r.n_agents);
            max_text = std::max(max_text, r.n_content);
        }
        DTGPU_CK(B->e_docs.upload(B->e_desc, s));
        DTGPU_CK(B->e_dres.alloc(B->n));
        DTGPU_CK(B->e_w.alloc(std::max<uint64_t>(w, 1)));
        DTGPU_CK(B->e_b.alloc(std::max<uint64_t>(b, 1)));
        DTGPU_CK(B->e_out.alloc(std::max<uint64_t>(o, 1)));
        EncParams &q = B->enc;
        q.in = Dd.in.p; q.content = Dd.content.p;
        q.aruns = Dd.aruns.p; q.ent = Dd.ent.p; q.poff = Dd.poff.p; q.par = Dd.par.p; q.cbyte = Dd.cbyte.p;
        q.agents = Dd.agents.p;
        q.cmds = B->d_cmds.p;
        q.w = B->e_w.p; q.b = B->e_b.p; q.out = B->e_out.p;
        q.docs = B->e_docs.p; q.results = B->e_dres.p;
        q.n_docs = uint32_t(B->n);
        q.max_agents = max_agents;
        // kernel 2 stages a document's text in LDS for the LZ4 pass when it fits: 16 KiB of hash
        // table + 512 B of output ring + <= 23.5 KiB of text keeps 4 waves per CU
        // measured (10k friendsforever): 60 ms with the text in LDS (4 waves per CU), 44 ms with
        // it read from HBM at 9 waves per CU -- occupancy wins in a batch, so staging is opt-in
        q.lds_text = 0;
        (void)max_text;
        q.lds_text = B->cfg.enc_lds_text;
        q.prof = B->cfg.enc_prof ? 1u : 0u;
        for (int k = 0; k < 32; k++) q.x2n[k] = Dd.P.x2n[k];
    }
    // the walk order: the planner's commands (prep + plan, as a checkout pass runs them), for
    // every document (a checkout pass skips the fast-forwarded ones: their lists cover the rest)
    {
        PrepParams pp = B->prep;
        PlanParams qq = B->plan;
        pp.doc_list = nullptr; pp.n_docs = uint32_t(B->n);
        qq.doc_list = nullptr; qq.n_docs = uint32_t(B->n);
        if (launch_prep(pp, s)) return DTGPU_ERR_HIP;
        if (B->n_gpu_planned && launch_plan(qq, s) != OK) return DTGPU_ERR_HIP;
    }
    B->enc.flags = flags;
    DTGPU_CK(hipMemsetAsync(B->e_dres.p, 0, std::max<size_t>(B->n, 1) * sizeof(EncResult), s));
    DTGPU_CK(hipEventRecord(B->ev0, s));
    if (launch_encode(B->enc, s)) return DTGPU_ERR_HIP;
    DTGPU_CK(hipEventRecord(B->ev1, s));
    B->e_res.resize(B->n);
    DTGPU_CK(hipMemcpyAsync(B->e_res.data(), B->e_dres.p, B->n * sizeof(EncResult), hipMemcpyDeviceToHost, s));
    DTGPU_CK(hipStreamSynchronize(s));
    float ms = 0;
    DTGPU_CK(hipEventElapsedTime(&ms, B->ev0, B->ev1));
    if (kernel_ms) *kernel_ms = ms;
    return DTGPU_OK;
}

dtgpu_status dtgpu_batch_encoded(const dtgpu_batch *B, size_t i, uint8_t *out, size_t cap, size_t *out_len,
                                 uint64_t prof[14]) {
    if (!B || i >= B->n || B->e_res.size() != B->n) return DTGPU_ERR_ARG;
    if (B->host_status[i] != OK) return dtgpu_status(B->host_status[i]);
    const EncResult &r = B->e_res[i];
    if (r.status != OK) return dtgpu_status(r.status);
    if (prof) {
        for (int k = 0; k < 6; k++) prof[k] = r.prof[k];
        for (int k = 0; k < 3; k++) prof[6 + k] = r.lzcyc[k];
        for (int k = 0; k < 3; k++) prof[9 + k] = r.lzst[k];
        prof[12] = r.prof[6];
        prof[13] = r.prof[7];
    }
    if (out_len) *out_len = r.len;
    if (!out) return DTGPU_OK;
    if (cap < r.len) return DTGPU_ERR_ARG;
    if (hipSetDevice(B->device) != hipSuccess) return DTGPU_ERR_HIP;
    if (hipMemcpy(out, B->e_out.p + B->e_desc[i].out_off, r.len, hipMemcpyDeviceToHost) != hipSuccess) return DTGPU_ERR_HIP;
    return DTGPU_OK;
}

uint64_t dtgpu_batch_encoded_bytes(const dtgpu_batch *B, int which) {
    if (!B || B->e_res.size() != B->n) return 0;
    uint64_t t = 0;
    for (size_t i = 0; i < B->n; i++) {
        if (B->host_status[i] != OK || B->e_res[i].status != OK) continue;
        const DecodeResult &r = B->dec->res[i];
        if (which == 0) t += B->e_res[i].len;
        else t += 16ull * r.n_ops + 8ull * r.n_entries + 4ull * r.n_parents + 16ull * r.n_aruns + r.n_content;
    }
    return t;
}

dtgpu_status dtgpu_batch_run(dtgpu_batch *B, void *stream) {
    if (!B) return DTGPU_ERR_ARG;
    if (hipSetDevice(B->device) != hipSuccess) return DTGPU_ERR_HIP;
    void *s = stream ? stream : reinterpret_cast<void *>(B->stream);
    if (B->debug)
        fprintf(stderr, "[dtgpu] launch lds tiers %u/%u/%u/%u (blocks %u/%u/%u/%u) hbm %u\n", B->tier[0].n_list,
                B->tier[1].n_list, B->tier[2].n_list, B->tier[3].n_list, B->tier[0].lds_blocks, B->tier[1].lds_blocks,
                B->tier[2].lds_blocks, B->tier[3].lds_blocks, B->large.n_list);
    if (B->debug) {
        size_t nc = 0;
        for (const DocDesc &d : B->docs) nc += (d.flags & DOC_CRITICAL) != 0;
        fprintf(stderr, "[dtgpu] critical %zu of %zu replays; split tier %d (%u + %u documents)\n", nc, B->docs.size(),
                B->split ? B->split_tier : -1, B->n_big, B->n_rest);
    }
    dtgpu_status st = dtgpu_status(launch_pass(B, reinterpret_cast<hipStream_t>(s)));
    if (!st) st = dtgpu_status(launch_blame_pass(B, reinterpret_cast<hipStream_t>(s)));
    if (B->debug) {
        fprintf(stderr, "[dtgpu] launched status %d\n", int(st));
        hipError_t e = hipStreamSynchronize(reinterpret_cast<hipStream_t>(s));
        fprintf(stderr, "[dtgpu] synced %d\n", int(e));
    }
    return st;
}
dtgpu_status dtgpu_batch_run_timed(dtgpu_batch *B, float *ms) {
    if (!B) return DTGPU_ERR_ARG;
    if (hipSetDevice(B->device) != hipSuccess) return DTGPU_ERR_HIP;
    // one checkout pass of the whole batch on its stream: for device-staged batches the walker
    // inputs (prep_kernel: parent entries, children CSR, chain decomposition -- what
    // SpanningTreeWalker::new builds inside checkout_tip, txn_trace.rs:114-188), then the walk
    // planner, then replay + materialisation
    hipStream_t s = B->stream;
    const bool prep = B->dec && !B->xf_mode;
    if (const int st = launch_pass(B, s, PassMarks{B->ev_prep, B->ev0, B->ev_mid})) return dtgpu_status(st);
    if (launch_blame_pass(B, s)) return DTGPU_ERR_HIP;   // (a blame batch: inside the pass's time)
    if (hipEventRecord(B->ev1, s) != hipSuccess) return DTGPU_ERR_HIP;
    if (hipEventSynchronize(B->ev1) != hipSuccess) return DTGPU_ERR_HIP;
    float t = 0, tp = 0, tq = 0;
    if (hipEventElapsedTime(&t, B->ev_prep, B->ev1) != hipSuccess) return DTGPU_ERR_HIP;
    if (hipEventElapsedTime(&tq, B->ev_prep, B->ev0) != hipSuccess) return DTGPU_ERR_HIP;
    if (hipEventElapsedTime(&tp, B->ev0, B->ev_mid) != hipSuccess) return DTGPU_ERR_HIP;
    B->last_prep_ms = prep ? tq : 0.0f;
    B->last_plan_ms = tp;
    B->last_replay_ms = t - tp - tq;
    if (ms) *ms = t;
    return DTGPU_OK;
}
extern "C++" dtgpu_status dtgpu::run_xf_pass(dtgpu_batch *B, float ms[3]) {
    if (!B || !B->xf_mode || !B->dec) return DTGPU_ERR_ARG;
    float t = 0;
    const dtgpu_status st = dtgpu_batch_run_timed(B, &t);
    if (st != DTGPU_OK) return st;
    ms[0] = t - B->last_plan_ms - B->last_replay_ms;
    ms[1] = B->last_plan_ms;
    ms[2] = B->last_replay_ms;
    return DTGPU_OK;
}
dtgpu_status dtgpu_batch_sync(dtgpu_batch *B) {
    if (!B) return DTGPU_ERR_ARG;
    return hipStreamSynchronize(B->stream) == hipSuccess ? DTGPU_OK : DTGPU_ERR_HIP;
}
size_t dtgpu_batch_size(const dtgpu_batch *B) { return B ? B->n : 0; }
dtgpu_status dtgpu_batch_last_times(const dtgpu_batch *B, float out[3]) {
    if (!B || !out) return DTGPU_ERR_ARG;
    out[0] = B->last_plan_ms;
    out[1] = B->last_replay_ms;
    out[2] = B->last_prep_ms;
    return DTGPU_OK;
}
size_t dtgpu_batch_segments(dtgpu_batch *B, size_t doc, uint32_t *out, size_t cap) {
    if (!B || doc >= B->n) return 0;
    for (const SegGroup &g : B->seg_groups) {
        if (B->seg_docs[g.first] != doc || g.count < 2) continue;   // (a blame batch's group of one: replayed whole)
        if (hipSetDevice(B->device) != hipSuccess) return 0;
        for (uint32_t k = 0; k < g.count && k < cap; k++) {
            const uint32_t d = B->seg_docs[g.first + k];
            DocDesc e{};   // the device descriptor: the pass's cut planning wrote the range
            DocResult r{};
            if (hipMemcpyAsync(&r, B->d_results.p + d, sizeof r, hipMemcpyDeviceToHost, B->stream) != hipSuccess ||
                hipMemcpyAsync(&e, B->d_docs.p + d, sizeof e, hipMemcpyDeviceToHost, B->stream) != hipSuccess ||
                hipStreamSynchronize(B->stream) != hipSuccess)
                return 0;
            uint32_t *w = out + 12 * size_t(k);
            const size_t slot = size_t(g.first) + k;
            const bool dev_cut = slot < B->seg_caps.size();   // device-staged: the pass plans the cuts
            w[8] = dev_cut && (e.flags & DOC_CUT_HOST) ? 1u : 0u;
            w[9] = dev_cut ? B->seg_caps[slot].lo : e.seg_lo;
            w[10] = dev_cut ? B->seg_caps[slot].hi : e.seg_hi;
            w[11] = dev_cut ? B->seg_caps[slot].u : e.seg_u;
            w[0] = e.seg_lo; w[1] = e.seg_hi; w[2] = e.seg_u;
            // the first segment's result slot is the document's: the combine step rewrote it
            w[3] = k ? r.status : 0u; w[4] = k ? r.out_len : 0u; w[5] = r.dbg[15];
            w[6] = r.lds; w[7] = r.n_blocks;
        }
        return g.count;
    }
    return 0;
}
size_t dtgpu_batch_host_planned(const dtgpu_batch *B, uint8_t *flags, size_t cap) {
    if (!B) return 0;
    if (flags) for (size_t i = 0; i < B->n && i < cap; i++) flags[i] = B->host_planned[i];
    size_t k = 0;
    for (uint8_t f : B->host_planned) k += f != 0;
    return k;
}
size_t dtgpu_batch_fast_forwarded(const dtgpu_batch *B, uint8_t *flags, size_t cap) {
    if (!B) return 0;
    if (flags) for (size_t i = 0; i < B->n && i < cap; i++) flags[i] = i < B->ff_doc.size() ? B->ff_doc[i] : 0;
    return B->n_ff;
}
size_t dtgpu_batch_late_pipelined(const dtgpu_batch *B, uint8_t *flags, size_t cap) {
    if (!B || !B->late_pipe) return 0;
    if (flags) for (size_t i = 0; i < B->n && i < cap; i++) flags[i] = B->late_doc[i];
    return B->n_late;
}
dtgpu_status dtgpu_batch_plan(dtgpu_batch *B, size_t i, uint32_t *cmds, size_t cmd_cap, uint32_t *tlist,
                              size_t tlist_cap, size_t *n_cmds, size_t *n_tlist) {
    if (!B || i >= B->n) return DTGPU_ERR_ARG;
    if (B->host_status[i] != OK) return dtgpu_status(B->host_status[i]);
    if (i < B->ff_doc.size() && B->ff_doc[i]) {   // fast-forwarded: a checkout pass plans no walk for it
        if (n_cmds) *n_cmds = 0;
        if (n_tlist) *n_tlist = 0;
        return DTGPU_OK;
    }
    const DocDesc &d = B->docs[i];
    std::vector<Cmd> c(d.ncmd);
    if (d.ncmd && hipMemcpyAsync(c.data(), B->d_cmds.p + d.cmd_off, d.ncmd * sizeof(Cmd), hipMemcpyDeviceToHost, B->stream) != hipSuccess)
        return DTGPU_ERR_HIP;
    if (hipStreamSynchronize(B->stream) != hipSuccess) return DTGPU_ERR_HIP;
    size_t nt = 0;
    for (const Cmd &x : c) if ((x.op & 15u) == CMD_TOG) nt = std::max<size_t>(nt, size_t(x.lv) + x.len);
    if (n_cmds) *n_cmds = c.size();
    if (n_tlist) *n_tlist = nt;
    if (cmds) {
        if (cmd_cap < c.size()) return DTGPU_ERR_ARG;
        std::memcpy(cmds, c.data(), c.size() * sizeof(Cmd));
    }
    if (tlist && nt) {
        if (tlist_cap < nt) return DTGPU_ERR_ARG;
        if (hipMemcpyAsync(tlist, B->d_tlist.p + d.tlist_off, nt * 4, hipMemcpyDeviceToHost, B->stream) != hipSuccess ||
            hipStreamSynchronize(B->stream) != hipSuccess)
            return DTGPU_ERR_HIP;
    }
    return DTGPU_OK;
}
uint64_t dtgpu_batch_algorithmic_bytes(dtgpu_batch *B) {
    if (!B) return 0;
    std::vector<dtgpu_doc_result> r(B->n);
    if (B->n && dtgpu_batch_results(B, r.data()) != DTGPU_OK) return 0;
    uint64_t out = 0;
    for (const auto &x : r) out += x.text_len;
    return B->alg_in_bytes + out;
}
dtgpu_status dtgpu_batch_plan_profile(dtgpu_batch *B, size_t i, uint64_t out[8]) {
    if (!B || i >= B->n || !out) return DTGPU_ERR_ARG;
    PlanResult r;
    if (hipMemcpyAsync(&r, B->p_results.p + i, sizeof r, hipMemcpyDeviceToHost, B->stream) != hipSuccess ||
        hipStreamSynchronize(B->stream) != hipSuccess)
        return DTGPU_ERR_HIP;
    for (int k = 0; k < 6; k++) out[k] = r.prof[k];
    out[6] = r.ncmd;
    out[7] = r.ntlist;
    return DTGPU_OK;
}
dtgpu_status dtgpu_batch_doc_stats(dtgpu_batch *B, size_t i, uint32_t out[29]) {
    if (!B || i >= B->docs.size() || !out) return DTGPU_ERR_ARG;   // (past n: the segment documents)
    DocResult r;
    if (hipMemcpyAsync(&r, B->d_results.p + i, sizeof r, hipMemcpyDeviceToHost, B->stream) != hipSuccess ||
        hipStreamSynchronize(B->stream) != hipSuccess)
        return DTGPU_ERR_HIP;
    out[0] = r.n_items; out[1] = r.n_blocks; out[2] = r.fail_cmd; out[3] = r.fail_site;
    out[4] = B->docs[i].ncmd; out[5] = B->docs[i].max_blocks;
    for (int k = 0; k < 16; k++) out[6 + k] = r.dbg[k];
    out[22] = r.n_sb;
    out[23] = r.lds;
    for (int k = 0; k < 3; k++) out[24 + k] = r.dbg[16 + k];
    out[27] = r.dbg[19];   // block loads that rebuilt stale masks
    out[28] = r.dbg[20];   // block loads (not from the registers' cached block)
    return DTGPU_OK;
}
dtgpu_status dtgpu_batch_lookup_stats(dtgpu_batch *B, size_t i, uint32_t out[2]) {
    if (!B || i >= B->docs.size() || !out) return DTGPU_ERR_ARG;
    DocResult r;
    if (hipMemcpyAsync(&r, B->d_results.p + i, sizeof r, hipMemcpyDeviceToHost, B->stream) != hipSuccess ||
        hipStreamSynchronize(B->stream) != hipSuccess)
        return DTGPU_ERR_HIP;
    out[0] = r.dbg[21];   // position lookups (inserts past position 0, delete rounds)
    out[1] = r.dbg[22];   // those the cached block answered
    return DTGPU_OK;
}
uint64_t dtgpu_batch_total_lv(const dtgpu_batch *B) { return B ? B->total_lv : 0; }

dtgpu_status dtgpu_batch_results(dtgpu_batch *B, dtgpu_doc_result *res) {
    if (!B || (!res && B->n)) return DTGPU_ERR_ARG;
    std::vector<DocResult> dr(B->n);
    if (B->n && hipMemcpyAsync(dr.data(), B->d_results.p, B->n * sizeof(DocResult), hipMemcpyDeviceToHost, B->stream) != hipSuccess)
        return DTGPU_ERR_HIP;
    if (hipStreamSynchronize(B->stream) != hipSuccess) return DTGPU_ERR_HIP;
    for (size_t i = 0; i < B->n; i++) {
        res[i].status = B->host_status[i] != OK ? B->host_status[i] : dr[i].status;
        res[i].reserved = 0;
        res[i].text_len = res[i].status == OK ? dr[i].out_len : 0;
        res[i].text_hash = res[i].status == OK ? dr[i].hash : 0;
        res[i].n_lv = B->n_lv[i];
    }
    return DTGPU_OK;
}
dtgpu_status dtgpu_batch_text(dtgpu_batch *B, size_t i, uint8_t *out, size_t cap, size_t *out_len) {
    if (!B || i >= B->n) return DTGPU_ERR_ARG;
    if (B->host_status[i] != OK) return dtgpu_status(B->host_status[i]);
    DocResult r;
    if (hipMemcpyAsync(&r, B->d_results.p + i, sizeof r, hipMemcpyDeviceToHost, B->stream) != hipSuccess ||
        hipStreamSynchronize(B->stream) != hipSuccess)
        return DTGPU_ERR_HIP;
    if (r.status != OK) {
        if (B->debug)
            fprintf(stderr, "[dtgpu] doc %zu status %u fail_cmd %u fail_site %u items %u blocks %u dbg %u %u %u %u %u %u %u %x %x %x\n", i, r.status,
                    r.fail_cmd, r.fail_site, r.n_items, r.n_blocks, r.dbg[0], r.dbg[1], r.dbg[2], r.dbg[3], r.dbg[4],
                    r.dbg[5], r.dbg[6], r.dbg[7], r.dbg[8], r.dbg[9]);
        return dtgpu_status(r.status);
    }
    if (out_len) *out_len = r.out_len;
    if (!out) return DTGPU_OK;
    if (cap < r.out_len) return DTGPU_ERR_ARG;
    if (r.out_len && (hipMemcpyAsync(out, B->d_out.p + B->docs[i].out_off, r.out_len, hipMemcpyDeviceToHost, B->stream) != hipSuccess ||
                      hipStreamSynchronize(B->stream) != hipSuccess))
        return DTGPU_ERR_HIP;
    return DTGPU_OK;
}
void dtgpu_batch_free(dtgpu_batch *B) { delete B; }

}  // extern "C"
