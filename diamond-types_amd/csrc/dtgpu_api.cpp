// dtgpu_api.cpp -- C ABI of libdtgpu (include/dtgpu.h): oplog handles, the oplogs a checkout at
// a version or over a projection runs on, and the batch constructors (staging itself is
// dtgpu_stage.cpp, the passes and read-back dtgpu_pass.cpp).  There is no CPU checkout path:
// without a HIP device every checkout call returns DTGPU_ERR_NO_DEVICE.
#include <cstring>
#include <queue>
#include <tuple>

#include "dt_batch.hpp"
#include "dt_summary.hpp"

using namespace dtgpu;

struct dtgpu_oplog {
    HostOpLog o;
    std::vector<uint64_t> last_added;   // the frontier the last decode_and_add reported
};

namespace {

void prepare_from_oplog(const HostOpLog &src, Prepared &p) {
    p.log = src;
    p.log.finish();
    p.status = build_plan(p.log, p.plan);
}
// Decoded oplog -> device planner input (the walk itself runs on the GPU).
void prepare_input(Prepared &p) {
    if (p.status == OK) p.status = build_plan_input(p.log, p.pi);
}

}  // namespace

extern "C" {

// ---- oplog ----------------------------------------------------------------------------------
dtgpu_status dtgpu_oplog_load(const uint8_t *bytes, size_t len, int ignore_crc, dtgpu_oplog **out) {
    if (!out || (!bytes && len)) return DTGPU_ERR_ARG;
    auto h = std::make_unique<dtgpu_oplog>();
    Status s = decode_dt(bytes, len, ignore_crc != 0, h->o);
    if (s != OK) { *out = nullptr; return dtgpu_status(s); }
    *out = h.release();
    return DTGPU_OK;
}
dtgpu_oplog *dtgpu_oplog_new(void) { return new dtgpu_oplog(); }
void dtgpu_oplog_free(dtgpu_oplog *o) { delete o; }
dtgpu_status dtgpu_oplog_decode_and_add(dtgpu_oplog *h, const uint8_t *bytes, size_t len, int ignore_crc,
                                        uint64_t *frontier, size_t cap, size_t *n_frontier) {
    if (!h || (!bytes && len) || (!frontier && cap)) return DTGPU_ERR_ARG;
    std::vector<uint64_t> f;
    const Status s = decode_and_add(bytes, len, ignore_crc != 0, h->o, f);
    if (s != OK) return dtgpu_status(s);
    for (size_t i = 0; i < f.size() && i < cap; i++) frontier[i] = f[i];
    if (n_frontier) *n_frontier = f.size();
    h->last_added = std::move(f);
    return DTGPU_OK;
}
size_t dtgpu_oplog_last_added_frontier(const dtgpu_oplog *h, uint64_t *out, size_t cap) {
    if (!h) return 0;
    for (size_t i = 0; i < h->last_added.size() && i < cap; i++) out[i] = h->last_added[i];
    return h->last_added.size();
}
int64_t dtgpu_oplog_doc_id(const dtgpu_oplog *h, char *out, size_t cap) {
    if (!h || !h->o.has_doc_id) return -1;
    if (out) std::memcpy(out, h->o.doc_id.data(), std::min(cap, h->o.doc_id.size()));
    return int64_t(h->o.doc_id.size());
}
dtgpu_status dtgpu_oplog_set_doc_id(dtgpu_oplog *h, const char *id, size_t len) {
    if (!h) return DTGPU_ERR_ARG;
    if (!id) { h->o.doc_id.clear(); h->o.has_doc_id = false; return DTGPU_OK; }
    if (!utf8_valid(reinterpret_cast<const uint8_t *>(id), len)) return DTGPU_ERR_ARG;
    h->o.doc_id.assign(id, len);
    h->o.has_doc_id = true;
    return DTGPU_OK;
}
int32_t dtgpu_oplog_get_or_create_agent_id(dtgpu_oplog *o, const char *name, size_t len) {
    if (!o || (!name && len)) return -1;
    return o->o.agent_id(name, len);
}
static bool parents_ok(const HostOpLog &o, const uint64_t *parents, size_t np) {
    for (size_t i = 0; i < np; i++) if (parents[i] >= o.n_lv) return false;
    return true;
}
int64_t dtgpu_oplog_add_insert_at(dtgpu_oplog *h, int32_t agent, const uint64_t *parents, size_t np,
                                  uint64_t pos, const char *utf8, size_t nbytes) {
    if (!h || agent < 0 || size_t(agent) >= h->o.agent_names.size() || !parents_ok(h->o, parents, np)) return -1;
    const uint8_t *s = reinterpret_cast<const uint8_t *>(utf8);
    if (nbytes && !utf8_valid(s, nbytes)) return -1;
    uint64_t nchars = 0;
    for (size_t i = 0; i < nbytes; i += utf8_len(s[i])) nchars++;
    const uint64_t start = h->o.n_lv;
    if (!nchars) return int64_t(start) - 1;
    h->o.push_ins(pos, s, nbytes, nchars, true);
    h->o.add_span(uint32_t(agent), std::vector<uint64_t>(parents, parents + np), start, start + nchars);
    return int64_t(start + nchars - 1);
}
int64_t dtgpu_oplog_add_delete_at(dtgpu_oplog *h, int32_t agent, const uint64_t *parents, size_t np,
                                  uint64_t del_start, uint64_t del_end) {
    if (!h || agent < 0 || size_t(agent) >= h->o.agent_names.size() || !parents_ok(h->o, parents, np)) return -1;
    const uint64_t start = h->o.n_lv;
    if (del_end <= del_start) return int64_t(start) - 1;
    h->o.push_del(del_start, del_end - del_start, true);
    h->o.add_span(uint32_t(agent), std::vector<uint64_t>(parents, parents + np), start, start + (del_end - del_start));
    return int64_t(h->o.n_lv - 1);
}
int64_t dtgpu_oplog_add_insert(dtgpu_oplog *h, int32_t agent, uint64_t pos, const char *utf8, size_t nbytes) {
    if (!h) return -1;
    std::vector<uint64_t> v = h->o.version;
    return dtgpu_oplog_add_insert_at(h, agent, v.data(), v.size(), pos, utf8, nbytes);
}
int64_t dtgpu_oplog_add_delete_without_content(dtgpu_oplog *h, int32_t agent, uint64_t s, uint64_t e) {
    if (!h) return -1;
    std::vector<uint64_t> v = h->o.version;
    return dtgpu_oplog_add_delete_at(h, agent, v.data(), v.size(), s, e);
}
size_t dtgpu_oplog_len(const dtgpu_oplog *h) { return h ? size_t(h->o.n_lv) : 0; }
size_t dtgpu_oplog_cut_ranges(const dtgpu_oplog *h, uint64_t *out, size_t cap) {
    if (!h) return 0;
    SegInput si;
    seg_input_from_log(h->o, si);
    const auto cuts = cut_ranges(si);
    for (size_t k = 0; k < cuts.size() && k < cap && out; k++) { out[2 * k] = cuts[k].first; out[2 * k + 1] = cuts[k].second; }
    return cuts.size();
}
size_t dtgpu_oplog_local_frontier(const dtgpu_oplog *h, uint64_t *out, size_t cap) {
    if (!h) return 0;
    for (size_t i = 0; i < h->o.version.size() && i < cap; i++) out[i] = h->o.version[i];
    return h->o.version.size();
}

// Graph::find_dominators_2 (src/causalgraph/graph/tools.rs:545-578): the frontier of the union
// of two versions -- the members not in the history of another member, ascending.
int64_t dtgpu_oplog_dominators(const dtgpu_oplog *h, const uint64_t *a, size_t na, const uint64_t *b, size_t nb,
                               uint64_t *out, size_t cap) {
    if (!h || (na && !a) || (nb && !b)) return -1;
    std::vector<uint64_t> u(a, a + na);
    u.insert(u.end(), b, b + nb);
    for (uint64_t v : u) if (v >= h->o.n_lv) return -1;
    std::sort(u.begin(), u.end());
    u.erase(std::unique(u.begin(), u.end()), u.end());
    std::vector<uint64_t> dom;
    std::vector<std::pair<uint64_t, uint64_t>> only_a, only_b;
    for (uint64_t v : u) {
        bool dominated = false;
        for (uint64_t w : u) {
            if (w <= v) continue;   // a version is only in the history of later LVs
            h->o.graph.diff_rev({v}, {w}, only_a, only_b);
            if (only_a.empty()) { dominated = true; break; }
        }
        if (!dominated) dom.push_back(v);
    }
    for (size_t i = 0; i < dom.size() && i < cap; i++) out[i] = dom[i];
    return int64_t(dom.size());
}

dtgpu_status dtgpu_oplog_plan_stats(const dtgpu_oplog *h, uint64_t out[4]) {
    if (!h || !out) return DTGPU_ERR_ARG;
    Prepared p;
    prepare_from_oplog(h->o, p);
    if (p.status != OK) return dtgpu_status(p.status);
    out[0] = p.plan.n_steps;
    out[1] = p.plan.n_retreat;
    out[2] = p.plan.n_advance;
    out[3] = p.plan.cmds.size();
    return DTGPU_OK;
}

size_t dtgpu_oplog_plan_commands(const dtgpu_oplog *h, uint32_t *cmds, size_t cap) {
    if (!h) return 0;
    Prepared p;
    prepare_from_oplog(h->o, p);
    if (p.status != OK) return 0;
    for (size_t i = 0; i < p.plan.cmds.size() && i < cap; i++) {
        cmds[4 * i] = p.plan.cmds[i].op;
        cmds[4 * i + 1] = p.plan.cmds[i].lv;
        cmds[4 * i + 2] = p.plan.cmds[i].len;
        cmds[4 * i + 3] = p.plan.cmds[i].pos;
    }
    return p.plan.cmds.size();
}

dtgpu_status dtgpu_oplog_encode(const dtgpu_oplog *h, const uint64_t *from, size_t n_from, uint32_t flags, uint8_t *out,
                                size_t cap, size_t *out_len) {
    if (!h || (n_from && !from)) return DTGPU_ERR_ARG;
    if (flags & ~uint32_t(DTGPU_ENCODE_FULL)) return DTGPU_ERR_ARG;   // see dtgpu.h
    std::vector<uint64_t> f(n_from + 1);
    const int64_t nf = dtgpu_oplog_dominators(h, from, n_from, nullptr, 0, f.data(), f.size());
    if (nf < 0) return DTGPU_ERR_ARG;
    f.resize(size_t(nf));
    std::vector<uint8_t> start, bytes;
    const bool with_start = (flags & DTGPU_ENCODE_STORE_START_BRANCH_CONTENT) && !f.empty();
    if (with_start) {   // ListBranch::new_at_local_version(self, from) (encode_oplog.rs:612-615), on the GPU
        size_t n = 0;   // the text is at most every inserted byte
        start.resize(h->o.ins_content.size() + 1);
        const dtgpu_status cs = dtgpu_checkout(h, f.data(), f.size(), start.data(), start.size(), &n);
        if (cs != DTGPU_OK) return cs;
        start.resize(n);
    }
    const Status st = encode_dt(h->o, f, (flags & DTGPU_ENCODE_STORE_INSERTED_CONTENT) != 0,
                                (flags & DTGPU_ENCODE_COMPRESS_CONTENT) != 0, with_start ? &start : nullptr, bytes);
    if (st != OK) return dtgpu_status(st);
    if (out_len) *out_len = bytes.size();
    if (!out) return DTGPU_OK;
    if (cap < bytes.size()) return DTGPU_ERR_ARG;
    std::memcpy(out, bytes.data(), bytes.size());
    return DTGPU_OK;
}

dtgpu_status dtgpu_lz4_compress(const uint8_t *in, size_t n, uint8_t *out, size_t cap, size_t *out_len) {
    if (!in && n) return DTGPU_ERR_ARG;
    std::vector<uint8_t> c;
    lz4_block_compress(in, n, c);
    if (out_len) *out_len = c.size();
    if (!out) return DTGPU_OK;
    if (cap < c.size()) return DTGPU_ERR_ARG;
    std::memcpy(out, c.data(), c.size());
    return DTGPU_OK;
}

size_t dtgpu_oplog_xf_order(const dtgpu_oplog *h, const uint64_t *from, size_t n_from, const uint64_t *merge,
                            size_t n_merge, uint32_t *out, size_t cap) {
    if (!h || (n_from && !from) || (n_merge && !merge)) return 0;
    HostOpLog log = h->o;
    log.finish();
    std::vector<uint64_t> f(n_from + 1), m(n_merge + 1);
    const int64_t nf = dtgpu_oplog_dominators(h, from, n_from, nullptr, 0, f.data(), f.size());
    const int64_t nm = dtgpu_oplog_dominators(h, merge, n_merge, nullptr, 0, m.data(), m.size());
    if (nf < 0 || nm < 0) return 0;
    f.resize(size_t(nf));
    m.resize(size_t(nm));
    Plan plan;
    size_t first = 0;
    if (build_xf_plan_from(log, f, m, plan, first) != OK) return 0;
    size_t k = 0;
    for (size_t i = first; i < plan.cmds.size(); i++) {
        const Cmd &c = plan.cmds[i];
        if ((c.op & 15u) == CMD_TOG) continue;
        for (uint32_t j = 0; j < c.len; j++, k++) if (k < cap) out[k] = c.lv + j;
    }
    return k;
}

size_t dtgpu_oplog_plan_tlist(const dtgpu_oplog *h, uint32_t *out, size_t cap) {
    if (!h) return 0;
    Prepared p;
    prepare_from_oplog(h->o, p);
    if (p.status != OK) return 0;
    if (out) std::memcpy(out, p.plan.tlist.data(), std::min(cap, p.plan.tlist.size()) * sizeof(uint32_t));
    return p.plan.tlist.size();
}

size_t dtgpu_oplog_ins_content(const dtgpu_oplog *h, uint8_t *out, size_t cap) {
    if (!h) return 0;
    const auto &c = h->o.ins_content;
    if (out) std::memcpy(out, c.data(), std::min(cap, c.size()));
    return c.size();
}
size_t dtgpu_oplog_char_offsets(const dtgpu_oplog *h, uint32_t *out, size_t cap) {
    if (!h) return 0;
    const auto &c = h->o.ins_cbyte;
    if (out) std::memcpy(out, c.data(), std::min(cap, c.size()) * sizeof(uint32_t));
    return c.size();
}
size_t dtgpu_oplog_agent_runs(const dtgpu_oplog *h, uint32_t *out, size_t cap) {
    if (!h) return 0;
    Prepared p;
    prepare_from_oplog(h->o, p);
    const auto &a = p.plan.agent_runs;
    if (out) std::memcpy(out, a.data(), std::min(cap, a.size()) * sizeof(uint32_t));
    return a.size();
}

size_t dtgpu_oplog_export(const dtgpu_oplog *h, int what, void *out, size_t cap) {
    if (!h) return 0;
    const HostOpLog &o = h->o;
    std::vector<uint32_t> w;
    std::vector<uint8_t> b;
    bool bytes = false;
    switch (what) {
        case DTGPU_EXPORT_OPS: {   // split at graph entries, as the decoders produce them
            HostOpLog f;
            f.ops = o.ops;
            f.graph = o.graph;
            f.finish();
            for (const OpRun &r : f.ops) {
                w.push_back(uint32_t(r.lv)); w.push_back(uint32_t(r.len)); w.push_back(uint32_t(r.pos));
                w.push_back(uint32_t(r.kind) | (uint32_t(r.fwd) << 1));
            }
            break;
        }
        case DTGPU_EXPORT_AGENT_RUNS:
            for (const AgentRun &r : o.agent_runs) {
                w.push_back(uint32_t(r.lv)); w.push_back(uint32_t(r.len)); w.push_back(r.agent); w.push_back(uint32_t(r.seq));
            }
            break;
        case DTGPU_EXPORT_ENTRIES:
            for (const GraphEntry &e : o.graph.entries) { w.push_back(uint32_t(e.start)); w.push_back(uint32_t(e.end)); }
            break;
        case DTGPU_EXPORT_PARENT_OFFSETS: {
            uint32_t k = 0;
            for (const GraphEntry &e : o.graph.entries) { w.push_back(k); k += uint32_t(e.parents.size()); }
            w.push_back(k);
            break;
        }
        case DTGPU_EXPORT_PARENTS:
            for (const GraphEntry &e : o.graph.entries) for (uint64_t p : e.parents) w.push_back(uint32_t(p));
            break;
        case DTGPU_EXPORT_CONTENT: b = o.ins_content; bytes = true; break;
        case DTGPU_EXPORT_CHAR_OFFSETS: w = o.ins_cbyte; break;
        case DTGPU_EXPORT_VERSION: for (uint64_t v : o.version) w.push_back(uint32_t(v)); break;
        case DTGPU_EXPORT_AGENT_NAMES:
            for (const std::string &nm : o.agent_names) { b.push_back(uint8_t(nm.size())); b.insert(b.end(), nm.begin(), nm.end()); }
            bytes = true;
            break;
        case DTGPU_EXPORT_DOC_ID:
            b.push_back(o.has_doc_id ? 1 : 0);
            if (o.has_doc_id) b.insert(b.end(), o.doc_id.begin(), o.doc_id.end());
            bytes = true;
            break;
        default: return 0;
    }
    const size_t per = what == DTGPU_EXPORT_OPS || what == DTGPU_EXPORT_AGENT_RUNS ? 4 : what == DTGPU_EXPORT_ENTRIES ? 2 : 1;
    if (bytes) {
        if (out) std::memcpy(out, b.data(), std::min(cap, b.size()));
        return b.size();
    }
    const size_t count = w.size() / per;
    if (out) std::memcpy(out, w.data(), std::min(cap, count) * per * 4);
    return count;
}

// ---- batch ----------------------------------------------------------------------------------
dtgpu_status dtgpu_batch_create(const uint8_t *const *docs, const size_t *lens, size_t n,
                                const dtgpu_batch_opts *opts, dtgpu_batch **out) {
    if (!out || (n && (!docs || !lens))) return DTGPU_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return DTGPU_ERR_NO_DEVICE;
    std::vector<Prepared> prep(n);
    const bool ignore_crc = opts && opts->ignore_crc;
    parallel_for(n, threads_for(opts, n), [&](size_t i) {
        Prepared &p = prep[i];
        p.status = decode_dt(docs[i], lens[i], ignore_crc, p.log);
        prepare_input(p);
    });
    return stage(prep, opts, out);
}
dtgpu_status dtgpu_batch_create_from_oplogs(const dtgpu_oplog *const *oplogs, size_t n,
                                            const dtgpu_batch_opts *opts, dtgpu_batch **out) {
    if (!out || (n && !oplogs)) return DTGPU_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return DTGPU_ERR_NO_DEVICE;
    std::vector<Prepared> prep(n);
    parallel_for(n, threads_for(opts, n), [&](size_t i) {
        prep[i].log = oplogs[i]->o;
        prep[i].log.finish();
        prepare_input(prep[i]);
    });
    return stage(prep, opts, out);
}
dtgpu_status dtgpu_batch_create_xf(const dtgpu_oplog *const *oplogs, size_t n, const dtgpu_batch_opts *opts,
                                   dtgpu_batch **out) {
    if (!out || (n && !oplogs)) return DTGPU_ERR_ARG;
    if (opts && (opts->flags & DTGPU_OPT_BLAME)) return DTGPU_ERR_ARG;   // blame is a checkout batch's
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return DTGPU_ERR_NO_DEVICE;
    std::vector<Prepared> prep(n);
    parallel_for(n, threads_for(opts, n), [&](size_t i) {
        prep[i].log = oplogs[i]->o;
        prep[i].log.finish();
        prep[i].xf_merge = prep[i].log.version;
        prepare_input(prep[i]);
    });
    return stage(prep, opts, out, true);
}
dtgpu_status dtgpu_batch_create_device(const uint8_t *const *docs, const size_t *lens, size_t n,
                                       const dtgpu_batch_opts *opts, dtgpu_batch **out) {
    if (!out || (n && (!docs || !lens))) return DTGPU_ERR_ARG;
    dtgpu_decoded *dh = nullptr;
    const dtgpu_status st = dtgpu_decode_create(docs, lens, n, opts, &dh);
    if (st != DTGPU_OK) return st;
    return stage_device(dh, opts, out);
}

dtgpu_status dtgpu_batch_create_decoded_opts(dtgpu_decoded *dec, const dtgpu_batch_opts *opts, dtgpu_batch **out) {
    if (!dec || !out) return DTGPU_ERR_ARG;
    if (!dec->stream && hipStreamCreateWithFlags(&dec->stream, hipStreamNonBlocking) != hipSuccess) {
        dtgpu_decode_free(dec);   // consumed on failure too (dtgpu.h)
        return DTGPU_ERR_HIP;
    }
    return stage_device(dec, opts, out);
}
dtgpu_status dtgpu_batch_create_decoded(dtgpu_decoded *dec, dtgpu_batch **out) {
    return dtgpu_batch_create_decoded_opts(dec, nullptr, out);
}

dtgpu_status dtgpu_batch_checkout(const uint8_t *const *docs, const size_t *lens, size_t n,
                                  const dtgpu_batch_opts *opts, dtgpu_doc_result *results) {
    dtgpu_batch *B = nullptr;
    dtgpu_status s = dtgpu_batch_create(docs, lens, n, opts, &B);
    if (s) return s;
    s = dtgpu_batch_run(B, nullptr);
    if (!s) s = dtgpu_batch_results(B, results);
    dtgpu_batch_free(B);
    return s;
}

// A sub-oplog's agents and ops: `s` starts as an oplog of o's agents and gets the agent runs and op
// runs of `o` inside the ascending LV ranges `rs`, clipped to them, at the LVs map(old LV).  (The
// caller adds the graph.)
static void copy_clipped(const HostOpLog &o, const std::vector<std::pair<uint64_t, uint64_t>> &rs,
                         const std::function<uint64_t(uint64_t)> &map, HostOpLog &s) {
    s = HostOpLog();
    s.agent_names = o.agent_names;
    s.agent_seqs.assign(o.agent_names.size(), {});
    size_t oi = 0, ai = 0;
    for (const auto &r : rs) {
        // agent assignment
        while (ai < o.agent_runs.size() && o.agent_runs[ai].lv + o.agent_runs[ai].len <= r.first) ai++;
        for (size_t k = ai; k < o.agent_runs.size() && o.agent_runs[k].lv < r.second; k++) {
            const AgentRun &a = o.agent_runs[k];
            const uint64_t x = std::max(a.lv, r.first), y = std::min(a.lv + a.len, r.second);
            if (x < y) s.assign(a.agent, a.seq + (x - a.lv), map(x), y - x);
        }
        // op runs, clipped (rev delete runs delete right to left: op_metrics.rs:184-202)
        while (oi < o.ops.size() && o.ops[oi].lv + o.ops[oi].len <= r.first) oi++;
        for (size_t k = oi; k < o.ops.size() && o.ops[k].lv < r.second; k++) {
            const OpRun &op = o.ops[k];
            const uint64_t x = std::max(op.lv, r.first), y = std::min(op.lv + op.len, r.second);
            if (x >= y) continue;
            if (op.kind == 0) {
                for (uint64_t u = x; u < y;) {   // pieces of uniform ContentIsKnown
                    const bool known = o.ins_cbyte[u] != ~0u;
                    uint64_t w = u + 1;
                    while (w < y && (o.ins_cbyte[w] != ~0u) == known) w++;
                    size_t b0 = 0, b1 = 0;
                    if (known) {
                        b0 = o.ins_cbyte[u];
                        b1 = o.ins_cbyte[w - 1] + utf8_len(o.ins_content[o.ins_cbyte[w - 1]]);
                    }
                    s.push_ins(op.pos + (u - op.lv), known ? o.ins_content.data() + b0 : nullptr, b1 - b0, w - u, known);
                    u = w;
                }
            } else if (op.fwd) {
                s.push_del(op.pos, y - x, true);
            } else {
                s.push_del(op.pos + (op.lv + op.len - y), y - x, false);
            }
        }
    }
}

// ListOpLog::checkout(&[LV]) (src/list/oplog.rs:32-36) is a merge from ROOT over the history of
// `version`.  That history is closed under parents, so it is an oplog of its own: its LVs are
// compacted in order (agents, seqs and op positions unchanged -- every op's position is relative
// to its parents' version, which lies inside the history) and its tip checkout is the checkout
// at `version`.  The sub-oplog is built here and checked out by the same device path.
static Status history_oplog(const HostOpLog &o, const std::vector<uint64_t> &version, HostOpLog &s) {
    for (uint64_t v : version) if (v >= o.n_lv) return ErrCheckout;
    std::vector<std::pair<uint64_t, uint64_t>> hist, none;
    o.graph.diff_rev(version, {}, hist, none);   // Hist(version), newest first
    std::reverse(hist.begin(), hist.end());
    std::vector<uint64_t> base(hist.size());      // new LV of each range's start
    uint64_t nn = 0;
    for (size_t i = 0; i < hist.size(); i++) { base[i] = nn; nn += hist[i].second - hist[i].first; }
    auto map = [&](uint64_t lv) -> uint64_t {      // old LV (inside the history) -> new LV
        size_t i = size_t(std::upper_bound(hist.begin(), hist.end(), lv,
                                           [](uint64_t v, const std::pair<uint64_t, uint64_t> &r) { return v < r.second; }) -
                          hist.begin());
        return base[i] + (lv - hist[i].first);
    };
    copy_clipped(o, hist, map, s);
    size_t ei = 0;
    for (const auto &r : hist) {
        // graph entries, clipped: a piece that starts inside an entry continues its previous LV
        while (ei < o.graph.entries.size() && o.graph.entries[ei].end <= r.first) ei++;
        for (size_t k = ei; k < o.graph.entries.size() && o.graph.entries[k].start < r.second; k++) {
            const GraphEntry &e = o.graph.entries[k];
            const uint64_t x = std::max(e.start, r.first), y = std::min(e.end, r.second);
            if (x >= y) continue;
            std::vector<uint64_t> par;
            if (x == e.start) for (uint64_t p : e.parents) par.push_back(map(p));
            else par.push_back(map(x - 1));
            std::sort(par.begin(), par.end());
            s.graph.push(par, map(x), map(y - 1) + 1);
        }
    }
    for (uint64_t v : version) s.version.push_back(map(v));
    std::sort(s.version.begin(), s.version.end());
    s.version.erase(std::unique(s.version.begin(), s.version.end()), s.version.end());
    if (s.n_lv != nn) return ErrCheckout;
    s.finish();
    return OK;
}

// TextInfo::merge_into's subgraph (src/listmerge/merge.rs:954-1054 via Graph::subgraph_raw and
// project_onto_subgraph_raw, src/causalgraph/graph/subgraph.rs:39-250): the ops of one text CRDT
// are the LV spans `T` of a shared causal graph; the text is checked out over the graph
// projected onto T, where a version's projection is the frontier of Hist(version) n T.  The
// sub-oplog is compacted like history_oplog (agents, seqs and positions kept: a text op's
// position is relative to that text alone), so the same device path checks it out.
static Status project_oplog(const HostOpLog &o, std::vector<std::pair<uint64_t, uint64_t>> spans, HostOpLog &s,
                            const std::vector<std::vector<uint64_t>> *extra = nullptr,
                            std::vector<std::vector<uint64_t>> *extra_out = nullptr) {
    std::sort(spans.begin(), spans.end());
    std::vector<std::pair<uint64_t, uint64_t>> t;   // merged, non-empty
    for (auto r : spans) {
        if (r.first > r.second || r.second > o.n_lv) return ErrArg;
        if (r.first == r.second) continue;
        if (!t.empty() && r.first <= t.back().second) t.back().second = std::max(t.back().second, r.second);
        else t.push_back(r);
    }
    std::vector<uint64_t> base(t.size());
    uint64_t nn = 0;
    for (size_t i = 0; i < t.size(); i++) { base[i] = nn; nn += t[i].second - t[i].first; }
    auto span_of = [&](uint64_t lv) -> int64_t {   // last span starting at or before lv
        return int64_t(std::upper_bound(t.begin(), t.end(), lv, [](uint64_t v, const std::pair<uint64_t, uint64_t> &r) {
                           return v < r.first; }) - t.begin()) - 1;
    };
    auto in_t = [&](uint64_t lv) { const int64_t i = span_of(lv); return i >= 0 && lv < t[size_t(i)].second; };
    auto map = [&](uint64_t lv) -> uint64_t { const int64_t i = span_of(lv); return base[size_t(i)] + (lv - t[size_t(i)].first); };
    copy_clipped(o, t, map, s);
    // The graph, in one pass over the entries cut into runs inside / outside T.  A run outside T
    // gets its projected version P (constant along the run: the chain below it); a run inside T
    // is an entry of the projected graph whose parents are the projection of its own parents.  A
    // projection is the union of the parents' P (a T member projects to itself), reduced to its
    // frontier in the projected graph built so far (it holds every earlier T member).
    // Projected versions can be wide antichains (a text whose ops hang off another's), so runs
    // share them and a union is reduced by one walk down the projected graph, newest entry first,
    // that stops below the union's lowest member (the reference's find_dominators heap walk,
    // src/causalgraph/graph/tools.rs:545-578).
    using Set = std::shared_ptr<const std::vector<uint64_t>>;
    struct Piece { uint64_t start, end; Set proj; };
    std::vector<Piece> outside;   // ascending
    std::vector<uint64_t> seen_to(1, 0);   // per projected entry: 1 + highest LV walked
    auto frontier_of = [&](std::vector<uint64_t> u) -> std::vector<uint64_t> {
        std::sort(u.begin(), u.end());
        u.erase(std::unique(u.begin(), u.end()), u.end());
        if (u.size() < 2) return u;
        const uint64_t lo = u.front();
        std::vector<uint8_t> dominated(u.size(), 0);
        std::priority_queue<uint64_t> heap;
        std::vector<size_t> touched;
        seen_to.resize(s.graph.entries.size(), 0);
        auto push_parents = [&](uint64_t x) {   // parents of LV x in the projected graph
            const int64_t ei = s.graph.find_idx(x);
            const GraphEntry &e = s.graph.entries[size_t(ei)];
            if (x > e.start) heap.push(x - 1);
            else for (uint64_t p : e.parents) heap.push(p);
        };
        for (uint64_t c : u) push_parents(c);
        while (!heap.empty()) {
            const uint64_t v = heap.top();
            heap.pop();
            if (v < lo) break;
            const size_t ei = size_t(s.graph.find_idx(v));
            if (seen_to[ei] > v) continue;
            const GraphEntry &e = s.graph.entries[ei];
            const uint64_t from = std::max(e.start, seen_to[ei]);   // [from, v] is new history
            if (!seen_to[ei]) touched.push_back(ei);
            seen_to[ei] = v + 1;
            for (auto it = std::lower_bound(u.begin(), u.end(), from); it != u.end() && *it <= v; ++it)
                dominated[size_t(it - u.begin())] = 1;
            if (from == e.start) for (uint64_t p : e.parents) heap.push(p);
        }
        for (size_t ei : touched) seen_to[ei] = 0;
        std::vector<uint64_t> dom;
        for (size_t i = 0; i < u.size(); i++) if (!dominated[i]) dom.push_back(u[i]);
        return dom;
    };
    auto project_set = [&](const std::vector<uint64_t> &ver) -> Set {
        std::vector<uint64_t> u;
        Set only;
        size_t sources = 0;
        for (uint64_t p : ver) {
            sources++;
            if (in_t(p)) { u.push_back(map(p)); continue; }
            auto it = std::upper_bound(outside.begin(), outside.end(), p,
                                       [](uint64_t v, const Piece &q) { return v < q.start; });
            if (it == outside.begin() || p >= (--it)->end) continue;   // cannot happen: parents precede
            only = it->proj;
            u.insert(u.end(), it->proj->begin(), it->proj->end());
        }
        if (sources == 1 && only) return only;   // one parent outside T: its run's projection
        return std::make_shared<const std::vector<uint64_t>>(frontier_of(std::move(u)));
    };
    auto project = [&](const std::vector<uint64_t> &ver) -> std::vector<uint64_t> { return *project_set(ver); };
    for (const GraphEntry &e : o.graph.entries) {
        for (uint64_t x = e.start; x < e.end;) {
            const bool inside = in_t(x);
            uint64_t y = x + 1;
            if (inside) {
                y = std::min(e.end, t[size_t(span_of(x))].second);
            } else {
                const int64_t i = span_of(x);   // next T span starts after x
                const size_t nx = size_t(i + 1);
                y = nx < t.size() ? std::min(e.end, t[nx].first) : e.end;
            }
            Set par = project_set(x == e.start ? e.parents : std::vector<uint64_t>{x - 1});
            if (inside) s.graph.push(*par, map(x), map(y - 1) + 1);
            else outside.push_back(Piece{x, y, std::move(par)});
            x = y;
        }
    }
    s.version = project(o.version);
    if (extra && extra_out) {   // further versions of the shared graph, projected the same way
        extra_out->clear();
        for (const auto &v : *extra) {
            for (uint64_t x : v) if (x >= o.n_lv) return ErrArg;
            extra_out->push_back(project(v));
        }
    }
    if (s.n_lv != nn) return ErrCheckout;
    s.finish();
    return OK;
}

dtgpu_status dtgpu_oplog_project(const dtgpu_oplog *h, const uint64_t *spans, size_t n_spans, dtgpu_oplog **out) {
    if (!h || !out || (n_spans && !spans)) return DTGPU_ERR_ARG;
    *out = nullptr;
    std::vector<std::pair<uint64_t, uint64_t>> t(n_spans);
    for (size_t i = 0; i < n_spans; i++) t[i] = {spans[2 * i], spans[2 * i + 1]};
    HostOpLog log = h->o;
    log.finish();   // op runs split at graph entries
    auto *sub = new dtgpu_oplog;
    const Status st = project_oplog(log, t, sub->o);
    if (st != OK) { delete sub; return dtgpu_status(st); }
    *out = sub;
    return DTGPU_OK;
}

int64_t dtgpu_oplog_project_version(const dtgpu_oplog *h, const uint64_t *spans, size_t n_spans, const uint64_t *version,
                                    size_t n_version, uint64_t *out, size_t cap) {
    if (!h || (n_spans && !spans) || (n_version && !version) || (cap && !out)) return -1;
    std::vector<std::pair<uint64_t, uint64_t>> t(n_spans);
    for (size_t i = 0; i < n_spans; i++) t[i] = {spans[2 * i], spans[2 * i + 1]};
    HostOpLog log = h->o;
    log.finish();
    HostOpLog sub;
    const std::vector<std::vector<uint64_t>> vs{std::vector<uint64_t>(version, version + n_version)};
    std::vector<std::vector<uint64_t>> pv;
    if (project_oplog(log, t, sub, &vs, &pv) != OK || pv.size() != 1) return -1;
    for (size_t i = 0; i < pv[0].size() && i < cap; i++) out[i] = pv[0][i];
    return int64_t(pv[0].size());
}

// AgentAssignment::local_to_agent_version (src/causalgraph/agent_assignment/mod.rs): the agent
// run holding lv, by binary search over the LV-ordered runs.
dtgpu_status dtgpu_oplog_local_to_remote(const dtgpu_oplog *h, uint64_t lv, uint32_t *agent, uint64_t *seq) {
    if (!h || !agent || !seq || lv >= h->o.n_lv) return DTGPU_ERR_ARG;
    const auto &r = h->o.agent_runs;
    auto it = std::upper_bound(r.begin(), r.end(), lv, [](uint64_t v, const AgentRun &a) { return v < a.lv; });
    if (it == r.begin()) return DTGPU_ERR_ARG;
    --it;
    if (lv >= it->lv + it->len) return DTGPU_ERR_ARG;
    *agent = it->agent;
    *seq = it->seq + (lv - it->lv);
    return DTGPU_OK;
}

// The local LV spans of the remote span (agent, seq .. seq + n), in seq order
// (AgentAssignment::remote_to_local_version over a span): binary search over the agent's runs,
// which are seq-ordered whenever the agent's ops arrived in seq order (a linear pass otherwise).
// Returns the span count, or -1 when part of the span is not in the oplog.
int64_t dtgpu_oplog_remote_to_local(const dtgpu_oplog *h, uint32_t agent, uint64_t seq, uint64_t n, uint64_t *spans,
                                    size_t cap) {
    if (!h || agent >= h->o.agent_seqs.size() || (cap && !spans)) return -1;
    const auto &v = h->o.agent_seqs[agent];
    const auto by_seq = [](const SeqRun &a, const SeqRun &b) { return a.seq < b.seq; };
    std::vector<SeqRun> hit;
    const uint64_t end = seq + n;
    if (std::is_sorted(v.begin(), v.end(), by_seq)) {
        auto it = std::upper_bound(v.begin(), v.end(), seq, [](uint64_t x, const SeqRun &r) { return x < r.seq; });
        if (it != v.begin()) --it;
        for (; it != v.end() && it->seq < end; ++it)
            if (it->seq + it->len > seq) hit.push_back(*it);
    } else {
        for (const SeqRun &r : v)
            if (r.seq < end && r.seq + r.len > seq) hit.push_back(r);
        std::sort(hit.begin(), hit.end(), by_seq);
    }
    size_t k = 0;
    uint64_t at = seq;
    for (const SeqRun &r : hit) {
        if (r.seq + r.len <= at) continue;
        if (r.seq > at) return -1;   // a gap: that seq is not known here
        const uint64_t hi = std::min(end, r.seq + r.len);
        if (k < cap) { spans[2 * k] = r.lv + (at - r.seq); spans[2 * k + 1] = r.lv + (hi - r.seq); }
        k++;
        at = hi;
    }
    return at == end ? int64_t(k) : -1;
}

// AgentAssignment::summarize_versions (src/causalgraph/summary.rs:119-132)
dtgpu_status dtgpu_oplog_summarize(const dtgpu_oplog *h, uint8_t *names, size_t names_cap, size_t *name_off,
                                   size_t *range_off, size_t entry_cap, uint64_t *ranges, size_t range_cap,
                                   size_t sizes[3]) {
    if (!h) return DTGPU_ERR_ARG;
    const HostOpLog &o = h->o;
    const auto by = summarize_runs(o.agent_names.size(), o.agent_runs.size(), [&](size_t i, uint32_t &a, uint64_t &seq, uint64_t &len) {
        a = o.agent_runs[i].agent; seq = o.agent_runs[i].seq; len = o.agent_runs[i].len;
    });
    const bool fit = write_summary(by, [&](size_t a, const uint8_t *&p, size_t &len) {
        p = reinterpret_cast<const uint8_t *>(o.agent_names[a].data()); len = o.agent_names[a].size();
    }, names, names_cap, name_off, range_off, entry_cap, ranges, range_cap, sizes);
    return fit ? DTGPU_OK : DTGPU_ERR_ARG;
}

// CausalGraph::intersect_with_summary (src/causalgraph/summary.rs:234-264) over
// intersect_with_summary_full (:175-208): the agent's runs in seq order, each one that overlaps a
// range a known piece counting with the LV of its last seq, every uncovered stretch a remainder
// record; then find_dominators over those LVs and the caller's.
dtgpu_status dtgpu_oplog_intersect_summary(const dtgpu_oplog *h, const dtgpu_summaries *s, size_t i, uint64_t *frontier,
                                           size_t frontier_cap, size_t *n_frontier, uint64_t *triples, size_t triple_cap,
                                           size_t *n_triples) {
    if (n_frontier) *n_frontier = 0;
    if (n_triples) *n_triples = 0;
    if (!h || !s || !s->entry_off || (!frontier && frontier_cap) || (!triples && triple_cap)) return DTGPU_ERR_ARG;
    const HostOpLog &o = h->o;
    const size_t e0 = s->entry_off[i], e1 = s->entry_off[i + 1];
    if (e1 < e0 || (e1 > e0 && (!s->name_off || !s->range_off))) return DTGPU_ERR_ARG;
    std::vector<uint64_t> lvs, rem;
    for (size_t e = e0; e < e1; e++) {
        if (s->name_off[e + 1] < s->name_off[e] || s->range_off[e + 1] < s->range_off[e]) return DTGPU_ERR_ARG;
        if ((s->name_off[e + 1] > s->name_off[e] && !s->names) || (s->range_off[e + 1] > s->range_off[e] && !s->ranges))
            return DTGPU_ERR_ARG;
        const std::string name(reinterpret_cast<const char *>(s->names) + s->name_off[e], s->name_off[e + 1] - s->name_off[e]);
        std::vector<AgentRun> runs;   // the named agent's runs, ascending seq
        for (size_t a = 0; a < o.agent_names.size(); a++) {
            if (o.agent_names[a] != name) continue;
            for (const AgentRun &r : o.agent_runs) if (r.agent == a) runs.push_back(r);
            break;
        }
        std::sort(runs.begin(), runs.end(), [](const AgentRun &a, const AgentRun &b) { return a.seq < b.seq; });
        for (size_t k = s->range_off[e]; k < s->range_off[e + 1]; k++) {
            const uint64_t rs = s->ranges[2 * k], re = s->ranges[2 * k + 1];
            if (rs >= re) return DTGPU_ERR_ARG;
            uint64_t next = rs;
            for (const AgentRun &r : runs) {
                if (r.seq >= re || r.seq + r.len <= rs) continue;
                const uint64_t ps = std::max(rs, r.seq), pe = std::min(re, r.seq + r.len);
                if (ps > next) rem.insert(rem.end(), {uint64_t(e - e0), next, ps});
                next = pe;
                lvs.push_back(r.lv + (pe - 1 - r.seq));
            }
            if (next < re) rem.insert(rem.end(), {uint64_t(e - e0), next, re});
        }
    }
    if (s->version_off) {
        if (s->version_off[i + 1] < s->version_off[i] || (s->version_off[i + 1] > s->version_off[i] && !s->versions))
            return DTGPU_ERR_ARG;
        lvs.insert(lvs.end(), s->versions + s->version_off[i], s->versions + s->version_off[i + 1]);
    }
    for (uint64_t v : lvs) if (v >= o.n_lv) return DTGPU_ERR_ARG;
    {   // a graph entry is a chain: only its highest LV here can be a dominator
        std::sort(lvs.begin(), lvs.end());
        std::vector<uint64_t> top;
        int64_t last = -1;
        for (size_t j = lvs.size(); j-- > 0;) {
            const int64_t e = o.graph.find_idx(lvs[j]);
            if (e != last) top.push_back(lvs[j]);
            last = e;
        }
        lvs.swap(top);
    }
    std::vector<uint64_t> dom(lvs.size() + 1);
    const int64_t nd = dtgpu_oplog_dominators(h, lvs.data(), lvs.size(), nullptr, 0, dom.data(), dom.size());
    if (nd < 0) return DTGPU_ERR_ARG;
    for (size_t k = 0; k < size_t(nd) && k < frontier_cap; k++) frontier[k] = dom[k];
    for (size_t k = 0; k < rem.size() && k < 3 * triple_cap; k++) triples[k] = rem[k];
    if (n_frontier) *n_frontier = size_t(nd);
    if (n_triples) *n_triples = rem.size() / 3;
    return DTGPU_OK;
}

dtgpu_status dtgpu_oplog_history(const dtgpu_oplog *h, const uint64_t *version, size_t n_version, dtgpu_oplog **out) {
    if (!h || !out || (n_version && !version)) return DTGPU_ERR_ARG;
    *out = nullptr;
    std::vector<uint64_t> v(n_version + 1);
    const int64_t nv = dtgpu_oplog_dominators(h, version, n_version, nullptr, 0, v.data(), v.size());
    if (nv < 0) return DTGPU_ERR_ARG;
    v.resize(size_t(nv));
    auto *sub = new dtgpu_oplog;
    const Status st = history_oplog(h->o, v, sub->o);
    if (st != OK) { delete sub; return dtgpu_status(st); }
    *out = sub;
    return DTGPU_OK;
}
dtgpu_status dtgpu_checkout(const dtgpu_oplog *h, const uint64_t *version, size_t n_version, uint8_t *out, size_t cap,
                            size_t *out_len) {
    if (!h || (n_version && !version)) return DTGPU_ERR_ARG;
    std::vector<uint64_t> v(n_version + 1);   // reduce to a frontier (Frontier::from_unsorted)
    const int64_t nv = dtgpu_oplog_dominators(h, version, n_version, nullptr, 0, v.data(), v.size());
    if (nv < 0) return DTGPU_ERR_CHECKOUT;
    v.resize(size_t(nv));
    dtgpu_oplog sub;
    const Status st = history_oplog(h->o, v, sub.o);
    if (st != OK) return dtgpu_status(st);
    return dtgpu_checkout_tip(&sub, out, cap, out_len);
}

dtgpu_status dtgpu_xf_operations_from(const dtgpu_oplog *h, const uint64_t *from, size_t n_from, const uint64_t *merge,
                                      size_t n_merge, uint32_t *out, size_t cap, size_t *n_out) {
    if (!h || (n_from && !from) || (n_merge && !merge)) return DTGPU_ERR_ARG;
    std::vector<Prepared> prep(1);
    Prepared &p = prep[0];
    p.log = h->o;
    p.log.finish();
    for (auto [v, n, dst] : {std::make_tuple(from, n_from, &p.xf_from), std::make_tuple(merge, n_merge, &p.xf_merge)}) {
        dst->resize(n + 1);   // reduce to frontiers (Frontier::from_unsorted)
        const int64_t k = dtgpu_oplog_dominators(h, v, n, nullptr, 0, dst->data(), dst->size());
        if (k < 0) return DTGPU_ERR_ARG;
        dst->resize(size_t(k));
    }
    {   // the reported LV count comes from the host plan (no GPU needed for a size query)
        Plan plan;
        size_t first = 0;
        const Status st = build_xf_plan_from(p.log, p.xf_from, p.xf_merge, plan, first);
        if (st != OK) return dtgpu_status(st);
        size_t k = 0;
        for (size_t i = first; i < plan.cmds.size(); i++) if ((plan.cmds[i].op & 15u) != CMD_TOG) k += plan.cmds[i].len;
        if (n_out) *n_out = k;
        if (!out) return DTGPU_OK;
        if (cap < k) return DTGPU_ERR_ARG;
        if (k == 0) return DTGPU_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return DTGPU_ERR_NO_DEVICE;
    prepare_input(p);
    dtgpu_batch *B = nullptr;
    dtgpu_status st = stage(prep, nullptr, &B, true);
    if (st) return st;
    std::unique_ptr<dtgpu_batch> hold(B);
    if (B->host_status[0] != OK) return dtgpu_status(B->host_status[0]);
    if (launch_replay_xf(B->large, B->stream) != OK) return DTGPU_ERR_HIP;
    DocResult r;
    std::vector<uint32_t> xfv(p.log.n_lv);
    if (hipMemcpyAsync(&r, B->d_results.p, sizeof r, hipMemcpyDeviceToHost, B->stream) != hipSuccess ||
        hipMemcpyAsync(xfv.data(), B->d_xf.p, xfv.size() * 4, hipMemcpyDeviceToHost, B->stream) != hipSuccess ||
        hipStreamSynchronize(B->stream) != hipSuccess)
        return DTGPU_ERR_HIP;
    if (r.status != OK) return dtgpu_status(r.status);
    // application order = the plan's reported INS / DEL commands in order
    size_t k = 0;
    for (size_t i = p.xf_first; i < p.plan.cmds.size(); i++) {
        const Cmd &c = p.plan.cmds[i];
        if ((c.op & 15u) == CMD_TOG) continue;
        for (uint32_t j = 0; j < c.len && k < cap; j++, k++) {
            out[2 * k] = c.lv + j;
            out[2 * k + 1] = xfv[c.lv + j];
        }
    }
    return DTGPU_OK;
}
dtgpu_status dtgpu_xf_operations(const dtgpu_oplog *h, uint32_t *out, size_t cap, size_t *n_out) {
    if (!h) return DTGPU_ERR_ARG;
    return dtgpu_xf_operations_from(h, nullptr, 0, h->o.version.data(), h->o.version.size(), out, cap, n_out);
}

dtgpu_status dtgpu_checkout_tip(const dtgpu_oplog *h, uint8_t *out, size_t cap, size_t *out_len) {
    if (!h) return DTGPU_ERR_ARG;
    dtgpu_batch *B = nullptr;
    dtgpu_status s = dtgpu_batch_create_from_oplogs(&h, 1, nullptr, &B);
    if (s) return s;
    s = dtgpu_batch_run(B, nullptr);
    size_t len = 0;
    if (!s) s = dtgpu_batch_text(B, 0, nullptr, 0, &len);
    if (!s) {
        if (out_len) *out_len = len;
        if (out) s = cap < len ? DTGPU_ERR_ARG : dtgpu_batch_text(B, 0, out, cap, &len);
    }
    dtgpu_batch_free(B);
    return s;
}

uint64_t dtgpu_text_hash(const uint8_t *t, size_t n) { return text_hash(t, n); }
int dtgpu_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
const char *dtgpu_status_str(dtgpu_status s) {
    static const char *names[] = {"OK", "InvalidMagic", "UnsupportedProtocolVersion", "DocIdMismatch",
                                  "BaseVersionUnknown", "UnknownChunk", "LZ4DecoderNeeded", "LZ4DecompressionError",
                                  "CompressedDataMissing", "InvalidChunkHeader", "MissingChunk", "InvalidLength",
                                  "UnexpectedEOF", "InvalidUTF8", "InvalidRemoteID", "InvalidVarInt", "InvalidContent",
                                  "GenericInvalidData", "ChecksumFailed", "DataMissing"};
    if (int(s) >= 0 && int(s) < 20) return names[s];
    switch (s) {
        case DTGPU_ERR_CHECKOUT: return "ErrCheckout";
        case DTGPU_ERR_CAPACITY: return "ErrCapacity";
        case DTGPU_ERR_HIP: return "ErrHip";
        case DTGPU_ERR_ARG: return "ErrArg";
        case DTGPU_ERR_NO_DEVICE: return "ErrNoDevice";
        default: return "Unknown";
    }
}

}  // extern "C"
