// dt_patch.hpp -- host/device layout of the batched patch encoder (dt_patch.hip):
// ListOpLog::encode_from(opts, from) (src/list/encoding/encode_oplog.rs:404-747) for a batch of
// (resident document, version) requests, one 64-lane wavefront per request.  The bytes equal
// dt_encode.cpp's (the host encoder) for the same document, frontier and options.
//
// Hist(from) holds a prefix of every graph entry (dt_history.hpp), so the new ops of an entry are
// its suffix [reach, end): at most one piece per entry.  Two launches, as the history projection
// has: patch_mark_kernel runs the history mark sweep (dt_mark.hpp), reduces the request to a
// frontier and counts the patch (pieces, LVs, parents, agent-run and op-run pieces, content bytes);
// the host sizes each request's scratch and output from those counts; patch_build_kernel walks
// the pieces in SpanningTreeWalker order, merges the records and writes the file.
#pragma once
#include <stdint.h>

#include "dt_history.hpp"

namespace dtgpu {

struct PatchCounts {          // patch_mark_kernel's result per request
    uint32_t status;          // 0, the base document's status, ErrArg, DECODE_DEFER
    uint32_t n_front;         // the reduced frontier's width (the LVs are in HistParams::o_front)
    uint32_t n_pieces;        // entries with new ops
    uint32_t n_lv;            // new LVs
    uint32_t n_par;           // parents of the pieces (1 for a piece that starts inside its entry)
    uint32_t n_ar;            // agent runs clipped to pieces
    uint32_t n_op;            // op runs clipped to pieces
    uint32_t n_text;          // known content bytes of the new inserts
    uint32_t n_names;         // bytes of an AgentNames chunk that lists every agent of the base
    uint32_t form;            // the mark words were in LDS (1) or in HBM scratch (2); 0: not marked
};

struct PatchResult {          // patch_build_kernel's result per request
    uint32_t status, len;
    uint32_t n_walk, n_op_runs, n_agent_runs, n_txns, n_mapped, text_len, lz_len, pad;
    uint32_t cyc[7];          // core-clock cycles (PatchParams::prof): pieces + edges, walk, records, op runs, text, LZ4, write + CRC
};

// Scratch of one request, laid out by the host from its counts (words: patch_words; bytes: patch_bytes).
struct PatchDesc {
    uint64_t w_off, b_off, out_off;   // words of PatchParams::w, bytes of ::b, bytes of ::out
    uint32_t out_cap, skip;           // skip: the status to report without building (0: build)
    uint32_t n_pieces, n_par, n_ar, n_op, n_lv, n_text, n_front;
    uint32_t c_oprec;                 // op records (after the ContentIsKnown splits)
    uint32_t c_aa, c_tx;              // bytes of the agent assignment / txn streams
    uint32_t doc_id_off, doc_id_len;  // in the base document's bytes (len ~0: none)
};

struct PatchParams {
    HistParams H;                     // the base arenas, the requests, the mark scratch (H.docs per request)
    const PatchDesc *docs;
    PatchCounts *counts;
    PatchResult *results;
    uint32_t *w;
    uint8_t *b, *out;
    uint32_t n_docs, flags;           // DTGPU_ENCODE_STORE_INSERTED_CONTENT | DTGPU_ENCODE_COMPRESS_CONTENT
    uint32_t lds_entries, prof;       // mark launch: words of dynamic LDS (the largest base kept there); prof: count phase cycles
    uint32_t x2n[32];                 // x^(2^k) mod the CRC-32C polynomial
};

// Bytes of a patch outside its streams, at most: 13 chunk headers of an id byte and a <= 5-byte
// length (CompressedFieldsLZ4, FileInfo, DocId, AgentNames, StartBranch, Version, Patches,
// PatchContent, Content / ContentCompressed, ContentIsKnown, OpVersions, OpTypeAndPosition,
// OpParents) = 78; the magic and protocol version 9; the CRC chunk 6; the LZ4 block's uncompressed
// length 5, the DocId's and the content's data type 1 + 1, PatchContent's kind 1, the compressed
// field's length 5 and the single ContentIsKnown run 5 = 18.
constexpr uint32_t PATCH_FIXED_BYTES = 78 + 9 + 6 + 18;   // 111
constexpr uint32_t PATCH_FRONT_BYTES = 10 * 64;   // the Version stream: two varints per frontier LV

// words of one request's scratch: see dt_patch.hip Scratch
inline uint64_t patch_words(uint32_t ne, uint32_t n_agents, const PatchDesc &d) {
    return uint64_t(ne) + 13ull * d.n_pieces + 2 + 3ull * d.n_par + 3ull * n_agents + 8ull * d.n_op + 4ull * d.c_oprec + 16;
}
inline uint64_t patch_lz_bound(uint64_t n) { return n + n / 255 + 16; }
inline uint64_t patch_bytes(const PatchDesc &d) {
    return uint64_t(d.c_aa) + d.c_tx + PATCH_FRONT_BYTES + 2ull * 16 + d.n_text + patch_lz_bound(d.n_text) + 64;
}

int launch_patch_mark(const PatchParams &p, void *stream);
int launch_patch_build(const PatchParams &p, void *stream);

}  // namespace dtgpu
