// dtgpu_merge.cpp -- C ABI of the batched merge over resident documents (include/dtgpu.h,
// dtgpu_decode_xf_from / dtgpu_merges_*): ListOpLog::iter_xf_operations_from and ListBranch::merge
// (src/list/merge.rs:24-95) for many (document, from, merging) requests in one call.
//
// The pass: project Hist(from u merging) of every request into an oplog of its own (dt_history.hip,
// entries kept as the base document's) -> `from` into projected LVs (dt_merge.hip) -> a
// device-staged transformed-ops batch over the projections (stage_device, xf form): prep ->
// plan_kernel_xf -> replay_xf -> the reported commands back into base LVs as records (dt_merge.hip).
// The host lays arenas out from counts and never sees an oplog or a plan.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "dt_batch.hpp"
#include "dt_merge.hpp"
#include "dt_request.hpp"

using namespace dtgpu;

struct dtgpu_merges {
    int device = 0;
    size_t n = 0;
    FrontierSet fronts;                   // n_front: 0 for a failed request and for a ROOT one
    std::vector<uint32_t> n_rec, ncmd, first;
    std::vector<uint64_t> rec_off;
    DevBuf<uint32_t> rec;                 // every request's records, {base lv, pos}
    DevBuf<uint32_t> from_proj;           // the requests' `from` in projected LVs (the batch's planner reads it)
    std::unique_ptr<dtgpu_batch> batch;   // the replayed projections: the merged texts live in its out arena
    uint32_t us[5] = {};
};

extern "C" {

dtgpu_status dtgpu_decode_xf_from(const dtgpu_decoded *base, const uint32_t *docs, const uint64_t *from,
                                  const size_t *from_off, const uint64_t *merging, const size_t *merging_off, size_t n,
                                  float *kernel_ms, dtgpu_merges **out) {
    if (out) *out = nullptr;
    if (!out || !request_ok(base, docs, from, from_off, n) || !sets_ok(merging, merging_off, n)) return DTGPU_ERR_ARG;
    DTGPU_CK(hipSetDevice(base->device));
    auto M = std::make_unique<dtgpu_merges>();
    M->device = base->device;
    M->n = n;
    M->n_rec.assign(n, 0); M->ncmd.assign(n, 0); M->first.assign(n, 0);
    M->rec_off.assign(n + 1, 0);
    if (kernel_ms) *kernel_ms = 0;
    if (!n) { *out = M.release(); return DTGPU_OK; }   // (an empty FrontierSet)

    // ---- 1. the projections: Hist(from u merging) of every request -------------------------------
    std::vector<uint64_t> uni;
    std::vector<size_t> uni_off(n + 1, 0);
    std::vector<uint32_t> fb;            // `from` per request: sorted, without repeats
    std::vector<uint64_t> fb_off(n + 1, 0);
    std::vector<uint8_t> root(n, 0);
    for (size_t i = 0; i < n; i++) {
        for (size_t k = from_off[i]; k < from_off[i + 1]; k++) uni.push_back(from[k]);
        for (size_t k = merging_off[i]; k < merging_off[i + 1]; k++) uni.push_back(merging[k]);
        uni_off[i + 1] = uni.size();
        root[i] = uni_off[i + 1] == uni_off[i];
        const size_t f0 = fb.size();
        for (size_t k = from_off[i]; k < from_off[i + 1]; k++) fb.push_back(lv32(from[k]));
        std::sort(fb.begin() + ptrdiff_t(f0), fb.end());
        fb.erase(std::unique(fb.begin() + ptrdiff_t(f0), fb.end()), fb.end());
        fb_off[i + 1] = fb.size();
    }
    HistKeep keep;
    dtgpu_decoded *H = nullptr;
    float ms_hist = 0;
    {
        const dtgpu_status st = decode_history(base, docs, uni.data(), uni_off.data(), n, &ms_hist, &H, &keep);
        if (st != DTGPU_OK) return st;
    }
    std::unique_ptr<dtgpu_decoded> hold(H);
    hipStream_t s = H->stream;
    // the merged version is the projection's reduced request (H goes on into the batch without it)
    M->fronts = std::move(H->fronts);
    std::vector<uint32_t> &status = M->fronts.status, &n_front = M->fronts.n_front;
    std::vector<uint32_t> ok(n, 0);
    for (size_t i = 0; i < n; i++) {
        if (status[i] == 0 && fb_off[i + 1] - fb_off[i] > MERGE_MAX_FROM) status[i] = DECODE_DEFER;
        ok[i] = status[i] == 0 && !root[i] ? 1u : 0u;
        if (!ok[i]) n_front[i] = 0;
    }

    // ---- 2. `from` in projected LVs ---------------------------------------------------------------
    Events<4> ev;
    DTGPU_CK(ev.create());
    DevBuf<uint32_t> d_fb, d_ok;
    DevBuf<uint32_t> &d_fp = M->from_proj;
    DevBuf<uint64_t> d_fboff;
    DTGPU_CK(d_fb.upload(fb, s)); DTGPU_CK(d_fp.alloc(fb.size())); DTGPU_CK(d_ok.upload(ok, s)); DTGPU_CK(d_fboff.upload(fb_off, s));
    MergeParams mp{};
    mp.b_ent = base->ent.p; mp.scr = keep.scr.p; mp.hd = keep.hd.p; mp.n = uint32_t(n);
    mp.from = d_fb.p; mp.from_out = d_fp.p; mp.from_off = d_fboff.p; mp.ok = d_ok.p;
    DTGPU_CK(ev.record(0, s));
    if (launch_merge_from(mp, s)) return DTGPU_ERR_HIP;
    DTGPU_CK(ev.record(1, s));
    DTGPU_CK(hipStreamSynchronize(s));

    // ---- 3. the transformed-ops batch over the projections ----------------------------------------
    XfStage xf;
    xf.d_from = d_fp.p;
    xf.from_off = fb_off;
    xf.skip.assign(n, 0);
    for (size_t i = 0; i < n; i++) xf.skip[i] = ok[i] ? 0 : 1;
    xf.xf_first.assign(n, 0);
    xf.n_xf.assign(n, 0);
    dtgpu_batch *B = nullptr;
    {
        const dtgpu_status st = stage_device(hold.release(), nullptr, &B, &xf);   // (consumes H)
        if (st != DTGPU_OK) return st;
    }
    M->batch.reset(B);
    s = B->stream;
    float pass[3] = {0, 0, 0};
    {
        const dtgpu_status st = run_xf_pass(B, pass);
        if (st != DTGPU_OK) return st;
    }
    std::vector<dtgpu_doc_result> dr(n);
    {
        const dtgpu_status st = dtgpu_batch_results(B, dr.data());
        if (st != DTGPU_OK) return st;
    }

    // ---- 4. the records, in base LVs ----------------------------------------------------------------
    std::vector<uint64_t> cmd_off(n, 0), lv_off(n, 0);
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++) {
        if (ok[i] && dr[i].status != 0) { status[i] = dr[i].status; ok[i] = 0; n_front[i] = 0; }
        M->rec_off[i] = total;
        if (!ok[i]) continue;
        const DocDesc &d = B->docs[i];
        cmd_off[i] = d.cmd_off; lv_off[i] = d.lv_off;
        M->ncmd[i] = d.ncmd; M->first[i] = std::min(xf.xf_first[i], d.ncmd); M->n_rec[i] = xf.n_xf[i];
        total += xf.n_xf[i];
    }
    M->rec_off[n] = total;
    DTGPU_CK(M->rec.alloc(2 * total));
    DevBuf<uint64_t> d_coff, d_lvoff, d_roff;
    DevBuf<uint32_t> d_ncmd, d_first, d_nrec;
    DTGPU_CK(d_coff.upload(cmd_off, s)); DTGPU_CK(d_lvoff.upload(lv_off, s)); DTGPU_CK(d_roff.upload(M->rec_off, s));
    DTGPU_CK(d_ncmd.upload(M->ncmd, s)); DTGPU_CK(d_first.upload(M->first, s)); DTGPU_CK(d_nrec.upload(M->n_rec, s));
    mp.cmds = B->d_cmds.p; mp.xf = B->d_xf.p;
    mp.cmd_off = d_coff.p; mp.lv_off = d_lvoff.p; mp.rec_off = d_roff.p;
    mp.ncmd = d_ncmd.p; mp.first = d_first.p; mp.n_rec = d_nrec.p;
    mp.rec = M->rec.p;
    DTGPU_CK(ev.record(2, s));
    if (launch_merge_records(mp, s)) return DTGPU_ERR_HIP;
    DTGPU_CK(ev.record(3, s));
    DTGPU_CK(hipStreamSynchronize(s));
    float t0 = 0, t1 = 0;
    DTGPU_CK(ev.ms(0, 1, &t0));
    DTGPU_CK(ev.ms(2, 3, &t1));
    M->us[0] = uint32_t(ms_hist * 1000.f);
    for (int k = 0; k < 3; k++) M->us[1 + k] = uint32_t(pass[k] * 1000.f);
    M->us[4] = uint32_t((t0 + t1) * 1000.f);
    if (kernel_ms) *kernel_ms = ms_hist + pass[0] + pass[1] + pass[2] + t0 + t1;
    *out = M.release();
    return DTGPU_OK;
}

size_t dtgpu_merges_size(const dtgpu_merges *m) { return m ? m->n : 0; }

dtgpu_status dtgpu_merges_result(const dtgpu_merges *m, size_t i, uint64_t *frontier, size_t cap, size_t *n_frontier) {
    if (n_frontier) *n_frontier = 0;
    return m ? m->fronts.read(i, frontier, cap, n_frontier) : DTGPU_ERR_ARG;
}

dtgpu_status dtgpu_merges_ops(const dtgpu_merges *m, size_t i, uint32_t *out, size_t cap, size_t *n_out) {
    if (n_out) *n_out = 0;
    if (!m || i >= m->n) return DTGPU_ERR_ARG;
    if (m->fronts.status[i]) return dtgpu_status(m->fronts.status[i]);
    const size_t k = m->n_rec[i];
    if (n_out) *n_out = k;
    if (!out) return DTGPU_OK;
    if (cap < k) return DTGPU_ERR_ARG;
    if (hipSetDevice(m->device) != hipSuccess) return DTGPU_ERR_HIP;
    if (k && hipMemcpy(out, m->rec.p + 2 * m->rec_off[i], k * 8, hipMemcpyDeviceToHost) != hipSuccess) return DTGPU_ERR_HIP;
    return DTGPU_OK;
}

dtgpu_status dtgpu_merges_text(const dtgpu_merges *m, size_t i, uint8_t *out, size_t cap, size_t *out_len) {
    if (out_len) *out_len = 0;
    if (!m || i >= m->n) return DTGPU_ERR_ARG;
    if (m->fronts.status[i]) return dtgpu_status(m->fronts.status[i]);
    if (!m->fronts.n_front[i]) return DTGPU_OK;   // the merged version is ROOT: the empty text
    if (hipSetDevice(m->device) != hipSuccess) return DTGPU_ERR_HIP;
    return dtgpu_batch_text(m->batch.get(), i, out, cap, out_len);
}

dtgpu_status dtgpu_merges_profile(const dtgpu_merges *m, size_t i, uint32_t out[8]) {
    if (!m || i >= m->n || !out) return DTGPU_ERR_ARG;
    for (int k = 0; k < 5; k++) out[k] = m->us[k];
    out[5] = m->ncmd[i]; out[6] = m->first[i]; out[7] = m->n_rec[i];
    return DTGPU_OK;
}

void dtgpu_merges_free(dtgpu_merges *m) { delete m; }

}  // extern "C"
