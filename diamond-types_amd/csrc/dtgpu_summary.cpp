// dtgpu_summary.cpp -- C ABI of the batched version-summary calls (include/dtgpu.h:
// dtgpu_decode_intersect, dtgpu_decode_encode_from_summaries, dtgpu_decode_summarize).
//
// Staging: the flattened summaries go to HBM as they are (offsets widened to 64 bits, one word per
// range naming its entry), the count launch of dt_summary.hip sizes every request, the LV-set, piece
// and remainder arenas are laid out from its counts, and the emit launch fills them.  The LV sets
// stay in HBM: dtgpu_decode_intersect runs the history mark launch over them for the frontiers,
// dtgpu_decode_encode_from_summaries hands them to the patch path (dt_request.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/dtgpu.h"
#include "dt_decoded.hpp"
#include "dt_request.hpp"
#include "dt_summary.hpp"

using namespace dtgpu;

// The result of a batch of intersections, on the host: statuses and frontiers, remainder records.
struct dtgpu_intersect {
    size_t n = 0;
    float count_ms = 0, emit_ms = 0, mark_ms = 0;
    FrontierSet fronts;
    std::vector<SumCounts> counts;
    std::vector<uint64_t> rem_off;        // per request, in triples
    std::vector<uint64_t> rem;
};

namespace {

// Everything the summary launches leave in HBM for what follows on the same stream.
struct Staged {
    MarkSetup setup;
    std::vector<SumDesc> sd;
    std::vector<SumCounts> counts;
    DevBuf<HistDesc> d_hd;
    DevBuf<SumDesc> d_sd;
    DevBuf<SumCounts> d_cnt;
    DevBuf<uint8_t> d_names;
    DevBuf<uint64_t> d_name_off, d_range_off, d_ranges, d_pieces, d_rem;
    DevBuf<uint32_t> d_range_ent, d_ext, d_eag, d_req;
    uint64_t rem_total = 0;
};

dtgpu_status check_summaries(const dtgpu_decoded *B, const dtgpu_summaries *s, size_t n) {
    if (!B || (n && (!s || !s->entry_off))) return DTGPU_ERR_ARG;
    if (!docs_ok(B->merged || B->ran, B->n, n ? s->doc : nullptr, n)) return DTGPU_ERR_ARG;
    if (!n) return DTGPU_OK;
    if (s->entry_off[0] != 0) return DTGPU_ERR_ARG;
    for (size_t i = 0; i < n; i++)
        if (s->entry_off[i + 1] < s->entry_off[i] || s->entry_off[i + 1] - s->entry_off[i] > 0x7FFFFFFFu) return DTGPU_ERR_ARG;
    const size_t ne = s->entry_off[n];
    if (ne && (!s->name_off || !s->range_off)) return DTGPU_ERR_ARG;
    if (ne && (s->name_off[0] != 0 || s->range_off[0] != 0)) return DTGPU_ERR_ARG;
    for (size_t e = 0; e < ne; e++)
        if (s->name_off[e + 1] < s->name_off[e] || s->range_off[e + 1] < s->range_off[e]) return DTGPU_ERR_ARG;
    if (ne && ((s->name_off[ne] && !s->names) || (s->range_off[ne] && !s->ranges))) return DTGPU_ERR_ARG;
    if (s->version_off) {   // the extra LVs: a request CSR that starts at 0, each set within a 31-bit count
        if (s->version_off[0] != 0 || !sets_ok(s->versions, s->version_off, n)) return DTGPU_ERR_ARG;
        for (size_t i = 0; i < n; i++)
            if (s->version_off[i + 1] - s->version_off[i] > 0x7FFFFFFFu) return DTGPU_ERR_ARG;
    }
    for (size_t i = 0; i < n && ne; i++)
        if (s->range_off[s->entry_off[i + 1]] - s->range_off[s->entry_off[i]] > 0x7FFFFFFFu) return DTGPU_ERR_ARG;
    return DTGPU_OK;
}

// Upload, count launch, arena layout, emit launch -- all on stream s; on return the LV sets
// (st.d_req, described by st.d_hd) are complete in stream order.  ev[0..1] bracket the count
// launch, ev[2..3] the emit launch.
dtgpu_status stage_summaries(const dtgpu_decoded *B, const dtgpu_summaries *s, size_t n, hipStream_t strm, Events<6> &ev,
                             Staged &st, SumParams &P) {
    mark_setup(*B, s->doc, n, st.setup);
    const size_t ne = n ? s->entry_off[n] : 0;
    const size_t nr = ne ? s->range_off[ne] : 0;
    std::vector<uint64_t> name_off(ne + 1, 0), range_off(ne + 1, 0);
    for (size_t e = 0; e <= ne && ne; e++) { name_off[e] = s->name_off[e]; range_off[e] = s->range_off[e]; }
    std::vector<uint8_t> names(ne ? s->name_off[ne] : 0);
    if (!names.empty()) std::memcpy(names.data(), s->names, names.size());
    std::vector<uint64_t> ranges(2 * nr);
    if (nr) std::memcpy(ranges.data(), s->ranges, 16 * nr);
    std::vector<uint32_t> range_ent(nr), ext;
    st.sd.assign(n, SumDesc{});
    if (s->version_off) pack_sets(s->versions, s->version_off, n, ext, st.sd.data(), &SumDesc::ext_off, &SumDesc::n_ext);
    uint64_t eag = 0;
    for (size_t i = 0; i < n; i++) {
        SumDesc &d = st.sd[i];
        d.ent0 = s->entry_off[i];
        d.n_ent = uint32_t(s->entry_off[i + 1] - s->entry_off[i]);
        d.rng0 = range_off[d.ent0];
        d.n_rng = uint32_t(range_off[d.ent0 + d.n_ent] - d.rng0);
        for (uint32_t e = 0; e < d.n_ent; e++)
            for (uint64_t k = range_off[d.ent0 + e]; k < range_off[d.ent0 + e + 1]; k++) range_ent[k] = e;
        d.skip = st.setup.hd[i].skip;
        d.eag_off = eag;
        eag += d.n_ent;
    }
    DTGPU_CK(st.d_names.upload(names, strm));
    DTGPU_CK(st.d_name_off.upload(name_off, strm));
    DTGPU_CK(st.d_range_off.upload(range_off, strm));
    DTGPU_CK(st.d_ranges.upload(ranges, strm));
    DTGPU_CK(st.d_range_ent.upload(range_ent, strm));
    DTGPU_CK(st.d_ext.upload(ext, strm));
    DTGPU_CK(st.d_eag.alloc(eag));
    DTGPU_CK(st.d_sd.upload(st.sd, strm));
    DTGPU_CK(st.d_hd.upload(st.setup.hd, strm));
    DTGPU_CK(st.d_cnt.alloc(n));
    P = SumParams{};
    hist_params_base(*B, P.H);
    P.H.docs = st.d_hd.p; P.H.n_docs = uint32_t(n);
    P.docs = st.d_sd.p; P.names = st.d_names.p; P.name_off = st.d_name_off.p; P.range_off = st.d_range_off.p;
    P.ranges = st.d_ranges.p; P.range_ent = st.d_range_ent.p; P.ext = st.d_ext.p; P.eag = st.d_eag.p;
    P.counts = st.d_cnt.p; P.n_docs = uint32_t(n);
    DTGPU_CK(ev.record(0, strm));
    if (launch_sum_count(P, strm)) return DTGPU_ERR_HIP;
    DTGPU_CK(ev.record(1, strm));
    st.counts.assign(n, SumCounts{});
    if (n) DTGPU_CK(hipMemcpyAsync(st.counts.data(), st.d_cnt.p, n * sizeof(SumCounts), hipMemcpyDeviceToHost, strm));
    DTGPU_CK(hipStreamSynchronize(strm));
    // the arenas, from the count launch's counts: an LV per known piece and per extra LV; the pieces
    // twice (a re-ordered range is ranked into the second half); a range of k pieces has at most
    // k + 1 uncovered stretches
    uint64_t req = 0, pc = 0, rem = 0;
    for (size_t i = 0; i < n; i++) {
        SumDesc &d = st.sd[i];
        HistDesc &h = st.setup.hd[i];
        const SumCounts &c = st.counts[i];
        if (c.status) d.skip = h.skip = c.status;
        if (!d.skip && uint64_t(c.n_known) + d.n_ext > 0x7FFFFFFFull) d.skip = h.skip = DTGPU_ERR_CAPACITY;
        if (d.skip) continue;
        d.c_known = c.n_known;
        d.c_rem = c.n_known + d.n_rng;
        h.req_off = req; h.n_req = c.n_known + d.n_ext;
        req += h.n_req;
        d.pc_off = pc; pc += 2ull * d.c_known;
        d.rem_off = rem; rem += d.c_rem;
    }
    st.rem_total = rem;
    DTGPU_CK(st.d_req.alloc(req));
    DTGPU_CK(st.d_pieces.alloc(2 * pc));
    DTGPU_CK(st.d_rem.alloc(3 * rem));
    if (n) DTGPU_CK(hipMemcpyAsync(st.d_sd.p, st.sd.data(), n * sizeof(SumDesc), hipMemcpyHostToDevice, strm));
    if (n) DTGPU_CK(hipMemcpyAsync(st.d_hd.p, st.setup.hd.data(), n * sizeof(HistDesc), hipMemcpyHostToDevice, strm));
    P.H.req = st.d_req.p; P.req = st.d_req.p; P.pieces = st.d_pieces.p; P.rem = st.d_rem.p;
    DTGPU_CK(ev.record(2, strm));
    if (launch_sum_emit(P, strm)) return DTGPU_ERR_HIP;
    DTGPU_CK(ev.record(3, strm));
    return DTGPU_OK;
}

// The emit launch's counts and remainder records to the host (enqueued; the caller synchronises).
dtgpu_status fetch_remainders(size_t n, hipStream_t strm, Staged &st, dtgpu_intersect &X) {
    X.n = n;
    X.counts.assign(n, SumCounts{});
    X.rem.assign(3 * st.rem_total, 0);
    X.rem_off.assign(n, 0);
    for (size_t i = 0; i < n; i++) X.rem_off[i] = st.sd[i].rem_off;
    if (n) DTGPU_CK(hipMemcpyAsync(X.counts.data(), st.d_cnt.p, n * sizeof(SumCounts), hipMemcpyDeviceToHost, strm));
    if (!X.rem.empty()) DTGPU_CK(hipMemcpyAsync(X.rem.data(), st.d_rem.p, X.rem.size() * 8, hipMemcpyDeviceToHost, strm));
    return DTGPU_OK;
}

}  // namespace

extern "C" {

dtgpu_status dtgpu_decode_intersect(const dtgpu_decoded *B, const dtgpu_summaries *s, size_t n, float *ms,
                                    dtgpu_intersect **out) {
    if (out) *out = nullptr;
    if (!out) return DTGPU_ERR_ARG;
    if (dtgpu_status st = check_summaries(B, s, n)) return st;
    DTGPU_CK(hipSetDevice(B->device));
    Stream own;
    Events<6> ev;   // the count launch's [0..1], the emit launch's [2..3], the mark launch's [4..5]
    DTGPU_CK(own.create());
    DTGPU_CK(ev.create());
    auto X = std::make_unique<dtgpu_intersect>();
    Staged st;
    SumParams P{};
    static const dtgpu_summaries none{};
    if (dtgpu_status r = stage_summaries(B, n ? s : &none, n, own.s, ev, st, P)) return r;
    // the history mark launch alone: it reduces each LV set to its dominators in o_front
    DevBuf<uint32_t> d_scr, d_ver, d_front;
    DevBuf<DecodeResult> d_res;
    DTGPU_CK(d_scr.alloc(st.setup.scr_words));
    DTGPU_CK(d_ver.alloc(uint64_t(DECODE_MAX_FRONTIER) * n));
    DTGPU_CK(d_front.alloc(uint64_t(DECODE_MAX_FRONTIER) * n));
    DTGPU_CK(d_res.alloc(n));
    HistParams H = P.H;
    H.scr = d_scr.p; H.o_ver = d_ver.p; H.o_front = d_front.p; H.results = d_res.p;
    H.lds_entries = st.setup.lds_entries;
    DTGPU_CK(ev.record(4, own.s));
    if (launch_hist_mark(H, own.s)) return DTGPU_ERR_HIP;
    DTGPU_CK(ev.record(5, own.s));
    std::vector<DecodeResult> res(n, DecodeResult{});
    if (n) DTGPU_CK(hipMemcpyAsync(res.data(), d_res.p, n * sizeof(DecodeResult), hipMemcpyDeviceToHost, own.s));
    if (dtgpu_status r = fetch_remainders(n, own.s, st, *X)) return r;
    DTGPU_CK(hipStreamSynchronize(own.s));
    DTGPU_CK(ev.ms(0, 1, &X->count_ms));
    DTGPU_CK(ev.ms(2, 3, &X->emit_ms));
    DTGPU_CK(fetch_frontiers(X->fronts, d_front.p, n));
    DTGPU_CK(ev.ms(4, 5, &X->mark_ms));
    for (size_t i = 0; i < n; i++) {
        X->fronts.status[i] = res[i].status;
        X->fronts.n_front[i] = res[i].status ? 0u : res[i].n_version;
    }
    if (ms) *ms = X->count_ms + X->emit_ms + X->mark_ms;
    *out = X.release();
    return DTGPU_OK;
}

dtgpu_status dtgpu_decode_encode_from_summaries(const dtgpu_decoded *B, const dtgpu_summaries *s, size_t n, uint32_t flags,
                                                float *ms, dtgpu_patches **patches, dtgpu_intersect **isect) {
    if (patches) *patches = nullptr;
    if (isect) *isect = nullptr;
    if (!patches || !isect) return DTGPU_ERR_ARG;
    if (flags & ~uint32_t(DTGPU_ENCODE_FULL)) return DTGPU_ERR_ARG;
    if (dtgpu_status st = check_summaries(B, s, n)) return st;
    DTGPU_CK(hipSetDevice(B->device));
    Stream own;
    Events<6> ev;
    DTGPU_CK(own.create());
    DTGPU_CK(ev.create());
    auto X = std::make_unique<dtgpu_intersect>();
    Staged st;
    SumParams P{};
    static const dtgpu_summaries none{};
    if (dtgpu_status r = stage_summaries(B, n ? s : &none, n, own.s, ev, st, P)) return r;
    if (dtgpu_status r = fetch_remainders(n, own.s, st, *X)) return r;
    float patch_ms = 0;
    dtgpu_patches *pp = nullptr;
    if (dtgpu_status r = patches_from_requests(B, n ? s->doc : nullptr, n, flags, st.setup, st.d_hd.p, st.d_req.p, own.s,
                                               &patch_ms, &pp, &X->fronts))
        return r;
    std::unique_ptr<dtgpu_patches, void (*)(dtgpu_patches *)> hold(pp, dtgpu_patches_free);
    DTGPU_CK(hipStreamSynchronize(own.s));
    DTGPU_CK(ev.ms(0, 1, &X->count_ms));
    DTGPU_CK(ev.ms(2, 3, &X->emit_ms));
    // (X->fronts: the frontiers are the patch path's mark launch's; a request that only the encoder
    // declined -- its status is in the patches -- still has its intersection)
    if (ms) *ms = X->count_ms + X->emit_ms + patch_ms;
    *patches = hold.release();
    *isect = X.release();
    return DTGPU_OK;
}

size_t dtgpu_intersect_size(const dtgpu_intersect *x) { return x ? x->n : 0; }

dtgpu_status dtgpu_intersect_result(const dtgpu_intersect *x, size_t i, uint64_t *frontier, size_t cap, size_t *n_frontier) {
    if (n_frontier) *n_frontier = 0;
    return x ? x->fronts.read(i, frontier, cap, n_frontier) : DTGPU_ERR_ARG;
}

dtgpu_status dtgpu_intersect_remainder(const dtgpu_intersect *x, size_t i, uint64_t *triples, size_t cap, size_t *n) {
    if (n) *n = 0;
    if (!x || i >= x->n || (!triples && cap)) return DTGPU_ERR_ARG;
    if (x->fronts.status[i]) return dtgpu_status(x->fronts.status[i]);
    const size_t k = x->counts[i].n_rem;
    if (n) *n = k;
    for (size_t j = 0; j < 3 * std::min(k, cap); j++) triples[j] = x->rem[3 * x->rem_off[i] + j];
    return DTGPU_OK;
}

dtgpu_status dtgpu_intersect_profile(const dtgpu_intersect *x, size_t i, uint32_t out[8]) {
    if (!x || i >= x->n || !out) return DTGPU_ERR_ARG;
    out[0] = x->counts[i].n_known; out[1] = x->counts[i].n_rem; out[2] = x->counts[i].n_resorted;
    out[3] = uint32_t(x->count_ms * 1000.f); out[4] = uint32_t(x->emit_ms * 1000.f); out[5] = uint32_t(x->mark_ms * 1000.f);
    out[6] = out[7] = 0;
    return DTGPU_OK;
}

void dtgpu_intersect_free(dtgpu_intersect *x) { delete x; }

// Host code over one copy of the document's agent runs, agents table and bytes (see dtgpu.h).
dtgpu_status dtgpu_decode_summarize(const dtgpu_decoded *B, size_t i, uint8_t *names, size_t names_cap, size_t *name_off,
                                    size_t *range_off, size_t entry_cap, uint64_t *ranges, size_t range_cap, size_t sizes[3]) {
    if (!B || i >= B->n || (!B->merged && !B->ran)) return DTGPU_ERR_ARG;
    const DecodeDesc &d = B->desc[i];
    const DecodeResult &r = B->res[i];
    if (r.status) return dtgpu_status(r.status);
    DTGPU_CK(hipSetDevice(B->device));
    std::vector<uint32_t> runs(4 * size_t(r.n_aruns)), agents(2 * size_t(r.n_agents));
    std::vector<uint8_t> in(d.in_len);
    if (!runs.empty()) DTGPU_CK(hipMemcpy(runs.data(), B->aruns.p + 4 * d.arun_off, runs.size() * 4, hipMemcpyDeviceToHost));
    if (!agents.empty()) DTGPU_CK(hipMemcpy(agents.data(), B->agents.p + 2 * d.agent_off, agents.size() * 4, hipMemcpyDeviceToHost));
    if (!in.empty()) DTGPU_CK(hipMemcpy(in.data(), B->in.p + d.in_off, in.size(), hipMemcpyDeviceToHost));
    const auto by = summarize_runs(r.n_agents, r.n_aruns, [&](size_t k, uint32_t &a, uint64_t &seq, uint64_t &len) {
        a = runs[4 * k + 2]; seq = runs[4 * k + 3]; len = runs[4 * k + 1];
    });
    const bool fit = write_summary(by, [&](size_t a, const uint8_t *&p, size_t &len) {
        const size_t off = agents[2 * a];
        len = agents[2 * a + 1];
        if (off + len > in.size()) len = 0;
        p = in.data() + (len ? off : 0);
    }, names, names_cap, name_off, range_off, entry_cap, ranges, range_cap, sizes);
    return fit ? DTGPU_OK : DTGPU_ERR_ARG;
}

}  // extern "C"
