// dt_history.hpp -- host/device layout of the batched history projection (dt_history.hip).
//
// ListOpLog::checkout(&[LV]) (src/list/oplog.rs:32-36) up to the replay: one 64-lane wavefront per
// output builds the history of a version of a resident (decoded) document as an oplog of its own,
// in the same SoA arenas the decoder writes (dt_decode.hpp).  The history is closed under parents,
// so it holds a prefix of every graph entry it touches: one word per base entry (`reach`, the end
// of that prefix) describes it, and an exclusive scan of the prefix lengths is the LV map.
//
// Two launches: hist_mark_kernel marks the history, reduces the request to a frontier and counts
// what the output needs (exact LVs and content bytes, upper bounds for the run arrays: the base
// records that intersect the history); the host lays the arenas out; hist_emit_kernel writes them
// with the host's RLE rules (HostOpLog::assign / push_ins / push_del / Graph::push / finish).
#pragma once
#include <stdint.h>

#include "dt_decode.hpp"

namespace dtgpu {

constexpr uint32_t HIST_ENT_WORDS = 4;          // per base entry of an output: reach, new base LV, content delta, head flag
constexpr uint32_t HIST_LDS_ENTRIES = 12288;    // entries whose mark words fit the wave's LDS (48 KiB)

struct HistDesc {
    // the resident document (a decoded handle's document): arena offsets in elements, counts
    uint64_t b_in, b_arun, b_op, b_ent, b_poff, b_par, b_content, b_lv, b_agent;
    uint32_t b_in_len, b_n_aruns, b_n_ops, b_n_ent, b_n_par, b_n_content, b_n_agents, b_n_lv;
    uint32_t b_complete, skip;   // skip: the status to report without projecting (0: project)
    // the request: LVs of the base document in HistParams::req
    uint64_t req_off;
    uint32_t n_req, use_lds;     // use_lds: the mark words live in LDS during the sweep (2: and it fences at agent scope)
    uint64_t scr_off;            // HIST_ENT_WORDS * b_n_ent words of HistParams::scr
    // output arenas (emit launch): offsets in elements and capacities
    uint64_t o_in, o_arun, o_op, o_ent, o_poff, o_par, o_content, o_lv, o_agent, o_ver;
    uint32_t c_arun, c_op, c_ent, c_par, c_content, c_lv, c_agent, c_in;
};

struct HistParams {
    const uint8_t *b_in, *b_content;
    const uint32_t *b_aruns, *b_ops, *b_ent, *b_poff, *b_par, *b_cbyte, *b_agents;
    const uint32_t *req;
    uint32_t *scr;
    uint8_t *o_in, *o_content;
    uint32_t *o_aruns, *o_ops, *o_ent, *o_poff, *o_par, *o_cbyte, *o_agents, *o_ver;
    uint32_t *o_front;           // per output DECODE_MAX_FRONTIER words: the reduced request (base LVs)
    const HistDesc *docs;
    // mark launch: n_lv, n_content exact; n_aruns, n_ops, n_entries, n_parents upper bounds;
    // n_version = the reduced frontier's width; prof[0] = 1 mark words in LDS, 2 in HBM.
    // emit launch: the final counts.
    DecodeResult *results;
    uint32_t n_docs, lds_entries;
    // 1: an included base entry is never joined to its predecessor, so the output's entries are the
    // base document's (clipped).  A walk over the output then visits what a walk over the base
    // document's spans visits, in the same order (the merge requests, dtgpu_merge.cpp).
    uint32_t keep_entries;
};

int launch_hist_mark(const HistParams &p, void *stream);
int launch_hist_emit(const HistParams &p, void *stream);

}  // namespace dtgpu
