// dtgpu_patch.cpp -- C ABI of the batched encode_from over resident documents (include/dtgpu.h,
// dtgpu_decode_encode_from / dtgpu_patches_*), and the patch path the summary calls share
// (patches_from_requests, dt_request.hpp).
//
// ListOpLog::encode_from(opts, from) for a batch (dt_patch.hip).  Staging as dtgpu_decode_history:
// the request CSR goes to HBM, the mark launch reduces every request and counts its patch, each
// request's scratch and output are laid out from those counts (patch_words / patch_bytes and the
// byte bound below), and the build launch writes the files.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <memory>
#include <vector>

#include "../../include/dtgpu.h"
#include "dt_decoded.hpp"
#include "dt_patch.hpp"
#include "dt_request.hpp"

using namespace dtgpu;

// dtgpu_decode_encode_from's result: the patches in one HBM arena (owned), each request's length,
// and in `fronts` its status and reduced frontier
struct dtgpu_patches {
    int device = 0;
    size_t n = 0;
    float mark_ms = 0, build_ms = 0;
    std::vector<PatchResult> res;
    std::vector<uint32_t> form;
    std::vector<uint64_t> out_off;
    FrontierSet fronts;
    DevBuf<uint8_t> out;
};

dtgpu_status dtgpu::patches_from_requests(const dtgpu_decoded *B, const uint32_t *doc, size_t n, uint32_t flags,
                                          const MarkSetup &setup, const HistDesc *d_hd, const uint32_t *d_req,
                                          hipStream_t s, float *ms, dtgpu_patches **out, FrontierSet *mark) {
    const std::vector<HistDesc> &hd = setup.hd;
    auto M = std::make_unique<dtgpu_patches>();
    M->device = B->device;
    M->n = n;
    Events<4> ev;
    DTGPU_CK(ev.create());
    DevBuf<uint32_t> d_scr, d_ver, d_front, d_w;
    DevBuf<uint8_t> d_b;
    DevBuf<PatchDesc> d_pd;
    DevBuf<PatchCounts> d_cnt;
    DevBuf<PatchResult> d_res;
    DTGPU_CK(d_scr.alloc(setup.scr_words));
    DTGPU_CK(d_ver.alloc(uint64_t(DECODE_MAX_FRONTIER) * n));
    DTGPU_CK(d_front.alloc(uint64_t(DECODE_MAX_FRONTIER) * n));
    DTGPU_CK(d_cnt.alloc(n));
    DTGPU_CK(d_res.alloc(n));
    PatchParams P{};
    HistParams &H = P.H;
    hist_params_base(*B, H);
    H.req = d_req; H.scr = d_scr.p; H.o_ver = d_ver.p; H.o_front = d_front.p;
    H.docs = d_hd; H.n_docs = uint32_t(n);
    P.counts = d_cnt.p; P.results = d_res.p; P.n_docs = uint32_t(n); P.lds_entries = setup.lds_entries;
    P.prof = getenv("DTGPU_PATCH_PROF") ? 1u : 0u;   // read at call time: the build waves count their phase cycles
    P.flags = flags & (DTGPU_ENCODE_STORE_INSERTED_CONTENT | DTGPU_ENCODE_COMPRESS_CONTENT);
    crc_x2n(P.x2n);
    DTGPU_CK(ev.record(0, s));
    if (launch_patch_mark(P, s)) return DTGPU_ERR_HIP;
    DTGPU_CK(ev.record(1, s));
    std::vector<PatchCounts> cnt(n, PatchCounts{});
    if (n) DTGPU_CK(hipMemcpyAsync(cnt.data(), d_cnt.p, n * sizeof(PatchCounts), hipMemcpyDeviceToHost, s));
    DTGPU_CK(hipStreamSynchronize(s));
    // scratch and output of every request, from the mark launch's counts
    std::vector<PatchDesc> pd(n, PatchDesc{});
    M->out_off.assign(n, 0);
    uint64_t words = 0, bytes = 0, outb = 0;
    for (size_t i = 0; i < n; i++) {
        const PatchCounts &c = cnt[i];
        const DecodeResult &br = B->res[doc[i]];
        PatchDesc &d = pd[i];
        d.skip = c.status;
        // the StartBranch content is the checkout at `from`: the host's dtgpu_oplog_encode has it
        if (!d.skip && c.n_front && (flags & DTGPU_ENCODE_STORE_START_BRANCH_CONTENT)) d.skip = DECODE_DEFER;
        if (d.skip) continue;
        d.n_pieces = c.n_pieces; d.n_par = c.n_par; d.n_ar = c.n_ar; d.n_op = c.n_op; d.n_lv = c.n_lv;
        d.n_text = c.n_text; d.n_front = c.n_front;
        d.doc_id_off = br.doc_id_off; d.doc_id_len = br.doc_id_len;
        // records: a ContentIsKnown change inside an op-run piece splits it (only where content is missing)
        const uint64_t oprec = uint64_t(c.n_op) + (hd[i].b_complete ? 0 : c.n_lv);
        // bytes: an agent assignment run is three varints of <= 5 bytes; a txn its length, then per
        // parent <= 5 bytes (local) or <= 10 (foreign agent and seq), 1 for ROOT; an op run <= 12
        // (a 36-bit head, a 33-bit diff); the Version two varints per frontier LV; the names chunk
        // lists at most every agent; PATCH_FIXED_BYTES covers the magic, the chunk headers and the CRC
        const uint64_t c_aa = 15ull * c.n_ar + 16, c_tx = 6ull * c.n_pieces + 10ull * c.n_par + 16;
        const uint64_t doc_id = br.doc_id_len == 0xFFFFFFFFu ? 0 : br.doc_id_len;
        const uint64_t cap = PATCH_FIXED_BYTES + patch_lz_bound(c.n_text) + c.n_names + doc_id + 10ull * c.n_front + c_aa + 12 * oprec + c_tx;
        if (oprec > 0x7FFFFFFFull || cap > 0x7FFFFFFFull) { d = PatchDesc{}; d.skip = DTGPU_ERR_CAPACITY; continue; }
        d.c_oprec = uint32_t(oprec); d.c_aa = uint32_t(c_aa); d.c_tx = uint32_t(c_tx); d.out_cap = uint32_t(cap);
        d.w_off = words; words += patch_words(hd[i].b_n_ent, hd[i].b_n_agents, d);
        d.b_off = bytes; bytes = (bytes + patch_bytes(d) + 15) & ~uint64_t(15);
        d.out_off = outb; outb = align256(outb + cap);
        M->out_off[i] = d.out_off;
    }
    DTGPU_CK(d_w.alloc(words));
    DTGPU_CK(d_b.alloc(bytes));
    DTGPU_CK(M->out.alloc(outb));
    DTGPU_CK(d_pd.upload(pd, s));
    P.docs = d_pd.p; P.w = d_w.p; P.b = d_b.p; P.out = M->out.p;
    DTGPU_CK(ev.record(2, s));
    if (launch_patch_build(P, s)) return DTGPU_ERR_HIP;
    DTGPU_CK(ev.record(3, s));
    M->res.assign(n, PatchResult{});
    if (n) DTGPU_CK(hipMemcpyAsync(M->res.data(), d_res.p, n * sizeof(PatchResult), hipMemcpyDeviceToHost, s));
    DTGPU_CK(hipStreamSynchronize(s));
    DTGPU_CK(fetch_frontiers(M->fronts, d_front.p, n));
    DTGPU_CK(ev.ms(0, 1, &M->mark_ms));
    DTGPU_CK(ev.ms(2, 3, &M->build_ms));
    // the frontier is the mark launch's: a request that only the encoder declined still has it
    M->form.assign(n, 0);
    for (size_t i = 0; i < n; i++) {
        M->fronts.n_front[i] = cnt[i].status ? 0u : cnt[i].n_front;
        M->fronts.status[i] = cnt[i].status;
        M->form[i] = cnt[i].form;
    }
    if (mark) {   // a set of its own for the fused call, with the mark launch's status
        DTGPU_CK(fetch_frontiers(*mark, d_front.p, n));
        mark->status = M->fronts.status;
        mark->n_front = M->fronts.n_front;
    }
    for (size_t i = 0; i < n; i++) M->fronts.status[i] = M->res[i].status;
    if (ms) *ms = M->mark_ms + M->build_ms;
    *out = M.release();
    return DTGPU_OK;
}

extern "C" {

dtgpu_status dtgpu_decode_encode_from(const dtgpu_decoded *B, const uint32_t *doc, const uint64_t *versions,
                                      const size_t *version_off, size_t n, uint32_t flags, float *ms,
                                      dtgpu_patches **out) {
    if (out) *out = nullptr;
    if (!out || !request_ok(B, doc, versions, version_off, n)) return DTGPU_ERR_ARG;
    if (flags & ~uint32_t(DTGPU_ENCODE_FULL)) return DTGPU_ERR_ARG;
    DTGPU_CK(hipSetDevice(B->device));
    Stream own;
    DTGPU_CK(own.create());
    MarkSetup setup;
    mark_setup(*B, doc, n, setup);
    std::vector<uint32_t> req;
    pack_sets(versions, version_off, n, req, setup.hd.data(), &HistDesc::req_off, &HistDesc::n_req);
    DevBuf<uint32_t> d_req;
    DevBuf<HistDesc> d_hd;
    DTGPU_CK(d_req.upload(req, own.s));
    DTGPU_CK(d_hd.upload(setup.hd, own.s));
    return patches_from_requests(B, doc, n, flags, setup, d_hd.p, d_req.p, own.s, ms, out);
}

size_t dtgpu_patches_size(const dtgpu_patches *p) { return p ? p->n : 0; }

dtgpu_status dtgpu_patches_result(const dtgpu_patches *p, size_t i, uint64_t *frontier, size_t cap, size_t *n_frontier) {
    if (n_frontier) *n_frontier = 0;
    return p ? p->fronts.read(i, frontier, cap, n_frontier) : DTGPU_ERR_ARG;
}

dtgpu_status dtgpu_patches_get(const dtgpu_patches *p, size_t i, uint8_t *out, size_t cap, size_t *out_len) {
    if (out_len) *out_len = 0;
    if (!p || i >= p->n) return DTGPU_ERR_ARG;
    const PatchResult &r = p->res[i];
    if (r.status) return dtgpu_status(r.status);
    if (out_len) *out_len = r.len;
    if (!out) return DTGPU_OK;
    if (cap < r.len) return DTGPU_ERR_ARG;
    if (r.len && hipMemcpy(out, p->out.p + p->out_off[i], r.len, hipMemcpyDeviceToHost) != hipSuccess) return DTGPU_ERR_HIP;
    return DTGPU_OK;
}

dtgpu_status dtgpu_patches_profile(const dtgpu_patches *p, size_t i, uint32_t out[12]) {
    if (!p || i >= p->n || !out) return DTGPU_ERR_ARG;
    const PatchResult &r = p->res[i];
    out[0] = p->form[i];
    out[1] = uint32_t(p->mark_ms * 1000.f);
    out[2] = uint32_t(p->build_ms * 1000.f);
    out[3] = r.n_walk;
    for (int k = 0; k < 7; k++) out[4 + k] = r.cyc[k];
    out[11] = 0;
    return DTGPU_OK;
}

void dtgpu_patches_free(dtgpu_patches *p) { delete p; }

}  // extern "C"
