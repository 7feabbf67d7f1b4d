// dt_request.cpp -- the base document's half of the history mark launch's descriptors, shared by
// every per-request call that runs the mark sweep (dt_request.hpp).
#include "dt_request.hpp"

#include <algorithm>
#include <cstdlib>

namespace dtgpu {

void hist_params_base(const dtgpu_decoded &B, HistParams &H) {
    H.b_in = B.in.p; H.b_content = B.content.p; H.b_aruns = B.aruns.p; H.b_ops = B.ops.p; H.b_ent = B.ent.p;
    H.b_poff = B.poff.p; H.b_par = B.par.p; H.b_cbyte = B.cbyte.p; H.b_agents = B.agents.p;
}

void mark_setup(const dtgpu_decoded &B, const uint32_t *doc, size_t n, MarkSetup &ms) {
    ms.hd.assign(n, HistDesc{});
    ms.scr_words = 0;
    ms.lds_entries = 0;
    // the mark words of a request live in LDS up to this many base entries, in its HBM scratch past
    // it (DTGPU_HISTORY_LDS_ENTRIES lowers the limit; 0: always HBM)
    uint32_t lds_cap = HIST_LDS_ENTRIES;
    const uint32_t lds_form = getenv("DTGPU_MARK_AGENT_FENCE") ? 2u : 1u;   // (measurement: the sweep's earlier fence)
    if (const char *e = getenv("DTGPU_HISTORY_LDS_ENTRIES")) lds_cap = uint32_t(std::min<unsigned long>(strtoul(e, nullptr, 10), HIST_LDS_ENTRIES));
    for (size_t i = 0; i < n; i++) {
        const DecodeDesc &bd = B.desc[doc[i]];
        const DecodeResult &br = B.res[doc[i]];
        HistDesc &h = ms.hd[i];
        h.skip = br.status;
        h.b_in = bd.in_off; h.b_arun = bd.arun_off; h.b_op = bd.op_off; h.b_ent = bd.ent_off; h.b_poff = bd.poff_off;
        h.b_par = bd.par_off; h.b_content = bd.content_off; h.b_lv = bd.lv_off; h.b_agent = bd.agent_off;
        if (br.status == 0) {
            h.b_in_len = bd.in_len; h.b_n_aruns = br.n_aruns; h.b_n_ops = br.n_ops; h.b_n_ent = br.n_entries;
            h.b_n_par = br.n_parents; h.b_n_content = br.n_content; h.b_n_agents = br.n_agents;
            h.b_n_lv = lv32(br.n_lv); h.b_complete = br.content_complete;
        }
        h.use_lds = h.b_n_ent <= lds_cap ? lds_form : 0u;
        if (h.use_lds && !h.skip) ms.lds_entries = std::max(ms.lds_entries, h.b_n_ent);
        h.scr_off = ms.scr_words;
        ms.scr_words += uint64_t(HIST_ENT_WORDS) * h.b_n_ent;
        h.o_ver = uint64_t(DECODE_MAX_FRONTIER) * i;
    }
}

}  // namespace dtgpu
