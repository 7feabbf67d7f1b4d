"""dt_amd -- Python mirror of diamond-types' `ListOpLog` / `ListBranch` checkout surface,
backed by libdtgpu (hand-written HIP kernels for MI355X, C ABI in include/dtgpu.h).

Mirrors (reference paths under jarrodhroberson/diamond-types):
  ListOpLog.load_from          src/list/encoding/decode_oplog.rs:447
  ListOpLog.checkout_tip       src/list/oplog.rs:38  (device replay: dt_replay.hip)
  ListOpLog.add_insert_at ...  src/list/oplog.rs:221-300
  ListBranch.content / len     src/list/branch.rs:38-63
  batch_checkout               SURVEY.md §8b batch entry

There is no CPU fallback: every checkout runs the HIP kernels, and a missing library or a
missing GPU raises immediately.
"""
import collections
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DTGPU_LIB_DIR: an alternative in-tree build (A/B experiments, e.g. lib_exp/); default lib/
LIB_PATH = os.path.join(os.path.dirname(_HERE), os.environ.get("DTGPU_LIB_DIR", "lib"), "libdtgpu.so")

STATUS_NAMES = {
    0: "OK", 1: "InvalidMagic", 2: "UnsupportedProtocolVersion", 3: "DocIdMismatch", 4: "BaseVersionUnknown",
    5: "UnknownChunk", 6: "LZ4DecoderNeeded", 7: "LZ4DecompressionError", 8: "CompressedDataMissing",
    9: "InvalidChunkHeader", 10: "MissingChunk", 11: "InvalidLength", 12: "UnexpectedEOF", 13: "InvalidUTF8",
    14: "InvalidRemoteID", 15: "InvalidVarInt", 16: "InvalidContent", 17: "GenericInvalidData",
    18: "ChecksumFailed", 19: "DataMissing", 64: "ErrCheckout", 65: "ErrCapacity", 66: "ErrHip", 67: "ErrArg",
    68: "ErrNoDevice",
}


class ParseError(Exception):
    """Mirror of `ParseError` (src/encoding/parseerror.rs:14-48) plus engine statuses."""

    def __init__(self, code):
        self.code = code
        self.name = STATUS_NAMES.get(code, str(code))
        super().__init__(f"{self.name} ({code})")


class DocResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("text_len", ctypes.c_uint64),
                ("text_hash", ctypes.c_uint64), ("n_lv", ctypes.c_uint64)]


class BatchOpts(ctypes.Structure):
    """dtgpu_batch_opts (include/dtgpu.h): flags = DTGPU_OPT_* (OPT_* below); seg_ops / seg_max /
    lds_fill 0 = defaults.  DTGPU_* environment variables override them at batch creation."""
    _fields_ = [("ignore_crc", ctypes.c_int), ("host_threads", ctypes.c_int), ("device", ctypes.c_int),
                ("flags", ctypes.c_uint32), ("seg_ops", ctypes.c_uint32), ("seg_max", ctypes.c_uint32),
                ("lds_fill", ctypes.c_uint32)]


OPT_NO_FAST_FORWARD, OPT_NO_SEGMENTS, OPT_HOST_PLAN, OPT_NO_SPLIT, OPT_NO_CRITICAL, OPT_DEBUG, OPT_PASS_MARK = \
    1, 2, 4, 8, 16, 32, 64
OPT_BLAME = 128   # the batch also produces each document's blame on every run (Batch.blame)


class BlameRun(ctypes.Structure):
    """dtgpu_blame_run (include/dtgpu.h): `len` characters of the text, character k inserted by LV
    lv + k = (agent, seq + k)."""
    _fields_ = [("lv", ctypes.c_uint32), ("len", ctypes.c_uint32), ("agent", ctypes.c_uint32), ("seq", ctypes.c_uint32)]


class GraphQuery(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_uint32), ("graph", ctypes.c_uint32), ("na", ctypes.c_size_t),
                ("nb", ctypes.c_size_t), ("a", ctypes.POINTER(ctypes.c_int64)), ("b", ctypes.POINTER(ctypes.c_int64)),
                ("target", ctypes.c_int64)]


class GraphAnswer(ctypes.Structure):
    _fields_ = [("status", ctypes.c_uint32), ("n_a", ctypes.c_uint32), ("n_b", ctypes.c_uint32),
                ("n_common", ctypes.c_uint32)]


_lib = None


class Summaries(ctypes.Structure):
    """dtgpu_summaries (include/dtgpu.h): a batch of version summaries, flattened."""
    _fields_ = [("doc", ctypes.POINTER(ctypes.c_uint32)), ("entry_off", ctypes.POINTER(ctypes.c_size_t)),
                ("names", ctypes.c_char_p), ("name_off", ctypes.POINTER(ctypes.c_size_t)),
                ("range_off", ctypes.POINTER(ctypes.c_size_t)), ("ranges", ctypes.POINTER(ctypes.c_uint64)),
                ("versions", ctypes.POINTER(ctypes.c_uint64)), ("version_off", ctypes.POINTER(ctypes.c_size_t))]


def _check_build_record():
    """The library's build record (lib/build_info.json, tools/build_info.py) names the hash of every
    source it was built from: a library built from other sources than the ones beside it (a stale
    prebuilt binary) is refused.  Experiment builds without a record (DTGPU_LIB_DIR) load as they are."""
    import hashlib
    import json
    info = os.path.join(os.path.dirname(LIB_PATH), "build_info.json")
    if not os.path.exists(info):
        return
    with open(info) as f:
        rec = json.load(f)
    pkg = os.path.dirname(os.path.dirname(LIB_PATH))
    stale = []
    for rel, h in rec.get("sources", {}).items():
        path = os.path.join(pkg, rel)
        if os.path.exists(path):
            with open(path, "rb") as f:
                if hashlib.sha256(f.read()).hexdigest() != h:
                    stale.append(rel)
    if stale:
        raise RuntimeError(f"{LIB_PATH} was built from other sources than {', '.join(stale[:4])}"
                           f"{' ...' if len(stale) > 4 else ''}; rebuild with `make -C diamond-types_amd`")


def lib():
    """Load libdtgpu.so (fails loudly when it has not been built, or was built from other sources)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"libdtgpu.so not built at {LIB_PATH}; run `make -C diamond-types_amd`")
    _check_build_record()
    L = ctypes.CDLL(LIB_PATH)
    vp, sz, u64, i64, c = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int
    pu64 = ctypes.POINTER(ctypes.c_uint64)
    L.dtgpu_oplog_load.argtypes = [ctypes.c_char_p, sz, c, ctypes.POINTER(vp)]
    L.dtgpu_oplog_new.restype = vp
    L.dtgpu_oplog_free.argtypes = [vp]
    L.dtgpu_oplog_get_or_create_agent_id.argtypes = [vp, ctypes.c_char_p, sz]
    L.dtgpu_oplog_get_or_create_agent_id.restype = ctypes.c_int32
    L.dtgpu_oplog_add_insert_at.argtypes = [vp, ctypes.c_int32, pu64, sz, u64, ctypes.c_char_p, sz]
    L.dtgpu_oplog_add_insert_at.restype = i64
    L.dtgpu_oplog_add_delete_at.argtypes = [vp, ctypes.c_int32, pu64, sz, u64, u64]
    L.dtgpu_oplog_add_delete_at.restype = i64
    L.dtgpu_oplog_add_insert.argtypes = [vp, ctypes.c_int32, u64, ctypes.c_char_p, sz]
    L.dtgpu_oplog_add_insert.restype = i64
    L.dtgpu_oplog_add_delete_without_content.argtypes = [vp, ctypes.c_int32, u64, u64]
    L.dtgpu_oplog_add_delete_without_content.restype = i64
    L.dtgpu_oplog_len.argtypes = [vp]
    L.dtgpu_oplog_len.restype = sz
    L.dtgpu_oplog_local_frontier.argtypes = [vp, pu64, sz]
    L.dtgpu_oplog_local_frontier.restype = sz
    L.dtgpu_oplog_plan_stats.argtypes = [vp, pu64]
    L.dtgpu_oplog_plan_commands.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), sz]
    L.dtgpu_oplog_plan_commands.restype = sz
    L.dtgpu_oplog_plan_tlist.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), sz]
    L.dtgpu_oplog_plan_tlist.restype = sz
    L.dtgpu_batch_last_times.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    L.dtgpu_batch_host_planned.argtypes = [vp, ctypes.POINTER(ctypes.c_uint8), sz]
    L.dtgpu_batch_host_planned.restype = sz
    L.dtgpu_batch_fast_forwarded.argtypes = [vp, ctypes.POINTER(ctypes.c_uint8), sz]
    L.dtgpu_batch_fast_forwarded.restype = sz
    L.dtgpu_batch_late_pipelined.argtypes = [vp, ctypes.POINTER(ctypes.c_uint8), sz]
    L.dtgpu_batch_late_pipelined.restype = sz
    pu32 = ctypes.POINTER(ctypes.c_uint32)
    L.dtgpu_batch_plan.argtypes = [vp, sz, pu32, sz, pu32, sz, ctypes.POINTER(sz), ctypes.POINTER(sz)]
    L.dtgpu_oplog_ins_content.argtypes = [vp, ctypes.c_char_p, sz]
    L.dtgpu_oplog_ins_content.restype = sz
    L.dtgpu_oplog_char_offsets.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), sz]
    L.dtgpu_oplog_char_offsets.restype = sz
    L.dtgpu_oplog_agent_runs.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), sz]
    L.dtgpu_oplog_agent_runs.restype = sz
    L.dtgpu_checkout_tip.argtypes = [vp, ctypes.c_char_p, sz, ctypes.POINTER(sz)]
    L.dtgpu_checkout.argtypes = [vp, pu64, sz, ctypes.c_char_p, sz, ctypes.POINTER(sz)]
    L.dtgpu_oplog_dominators.argtypes = [vp, pu64, sz, pu64, sz, pu64, sz]
    L.dtgpu_oplog_dominators.restype = ctypes.c_int64
    L.dtgpu_oplog_history.argtypes = [vp, pu64, sz, ctypes.POINTER(vp)]
    L.dtgpu_oplog_project.argtypes = [vp, pu64, sz, ctypes.POINTER(vp)]
    L.dtgpu_oplog_project_version.argtypes = [vp, pu64, sz, pu64, sz, pu64, sz]
    L.dtgpu_oplog_project_version.restype = i64
    L.dtgpu_oplog_local_to_remote.argtypes = [vp, u64, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(u64)]
    L.dtgpu_oplog_remote_to_local.argtypes = [vp, ctypes.c_uint32, u64, u64, pu64, sz]
    L.dtgpu_oplog_remote_to_local.restype = i64
    L.dtgpu_oplog_encode.argtypes = [vp, pu64, sz, ctypes.c_uint32, ctypes.c_char_p, sz, ctypes.POINTER(sz)]
    L.dtgpu_lz4_compress.argtypes = [ctypes.c_char_p, sz, ctypes.c_char_p, sz, ctypes.POINTER(sz)]
    L.dtgpu_oplog_decode_and_add.argtypes = [vp, ctypes.c_char_p, sz, c, pu64, sz, ctypes.POINTER(sz)]
    L.dtgpu_oplog_last_added_frontier.argtypes = [vp, pu64, sz]
    L.dtgpu_oplog_last_added_frontier.restype = sz
    L.dtgpu_oplog_doc_id.argtypes = [vp, ctypes.c_char_p, sz]
    L.dtgpu_oplog_doc_id.restype = ctypes.c_int64
    L.dtgpu_oplog_set_doc_id.argtypes = [vp, ctypes.c_char_p, sz]
    L.dtgpu_xf_operations.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), sz, ctypes.POINTER(sz)]
    L.dtgpu_oplog_xf_order.argtypes = [vp, pu64, sz, pu64, sz, ctypes.POINTER(ctypes.c_uint32), sz]
    L.dtgpu_oplog_xf_order.restype = sz
    L.dtgpu_xf_operations_from.argtypes = [vp, pu64, sz, pu64, sz, ctypes.POINTER(ctypes.c_uint32), sz,
                                           ctypes.POINTER(sz)]
    L.dtgpu_batch_create.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(sz), sz,
                                     ctypes.POINTER(BatchOpts), ctypes.POINTER(vp)]
    L.dtgpu_batch_create_from_oplogs.argtypes = [ctypes.POINTER(vp), sz, ctypes.POINTER(BatchOpts), ctypes.POINTER(vp)]
    L.dtgpu_batch_create_xf.argtypes = [ctypes.POINTER(vp), sz, ctypes.POINTER(BatchOpts), ctypes.POINTER(vp)]
    L.dtgpu_batch_xf_positions.argtypes = [vp, sz, ctypes.POINTER(ctypes.c_uint32), sz, ctypes.POINTER(sz)]
    L.dtgpu_batch_run.argtypes = [vp, vp]
    L.dtgpu_batch_run_timed.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    L.dtgpu_batch_sync.argtypes = [vp]
    L.dtgpu_batch_size.argtypes = [vp]
    L.dtgpu_batch_size.restype = sz
    L.dtgpu_batch_results.argtypes = [vp, ctypes.POINTER(DocResult)]
    L.dtgpu_batch_text.argtypes = [vp, sz, ctypes.c_char_p, sz, ctypes.POINTER(sz)]
    L.dtgpu_batch_algorithmic_bytes.argtypes = [vp]
    L.dtgpu_batch_algorithmic_bytes.restype = u64
    L.dtgpu_batch_doc_stats.argtypes = [vp, sz, ctypes.POINTER(ctypes.c_uint32)]
    L.dtgpu_batch_lookup_stats.argtypes = [vp, sz, ctypes.POINTER(ctypes.c_uint32)]
    L.dtgpu_batch_segments.argtypes = [vp, sz, ctypes.POINTER(ctypes.c_uint32), sz]
    L.dtgpu_batch_segments.restype = sz
    L.dtgpu_oplog_cut_ranges.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), sz]
    L.dtgpu_oplog_cut_ranges.restype = sz
    L.dtgpu_batch_plan_profile.argtypes = [vp, sz, ctypes.POINTER(ctypes.c_uint64)]
    L.dtgpu_batch_total_lv.argtypes = [vp]
    L.dtgpu_batch_total_lv.restype = u64
    L.dtgpu_batch_free.argtypes = [vp]
    L.dtgpu_batch_create_device.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(sz), sz,
                                            ctypes.POINTER(BatchOpts), ctypes.POINTER(vp)]
    L.dtgpu_batch_run_e2e_timed.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    L.dtgpu_batch_encode.argtypes = [vp, ctypes.c_uint32, ctypes.POINTER(ctypes.c_float)]
    L.dtgpu_batch_encoded.argtypes = [vp, sz, ctypes.c_char_p, sz, ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_uint64)]
    L.dtgpu_batch_encoded_bytes.argtypes = [vp, ctypes.c_int]
    L.dtgpu_batch_encoded_bytes.restype = ctypes.c_uint64
    L.dtgpu_batch_checkout.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(sz), sz,
                                       ctypes.POINTER(BatchOpts), ctypes.POINTER(DocResult)]
    L.dtgpu_text_hash.argtypes = [ctypes.c_char_p, sz]
    L.dtgpu_text_hash.restype = u64
    L.dtgpu_device_count.restype = c
    L.dtgpu_synth_ops.argtypes = [u64, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), sz]
    L.dtgpu_synth_ops.restype = sz
    L.dtgpu_synth_oplog.argtypes = [u64, ctypes.c_uint32, ctypes.POINTER(vp)]
    L.dtgpu_synth_merge_oplog.argtypes = [u64, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(vp)]
    L.dtgpu_oplog_export.argtypes = [vp, c, vp, sz]
    L.dtgpu_oplog_export.restype = sz
    L.dtgpu_decode_create.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(sz), sz,
                                      ctypes.POINTER(BatchOpts), ctypes.POINTER(vp)]
    L.dtgpu_decode_run.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    L.dtgpu_decode_size.argtypes = [vp]
    L.dtgpu_decode_size.restype = sz
    L.dtgpu_decode_status.argtypes = [vp, sz, pu64]
    L.dtgpu_decode_export.argtypes = [vp, sz, c, vp, sz]
    L.dtgpu_decode_export.restype = sz
    L.dtgpu_decode_bytes.argtypes = [vp, c]
    L.dtgpu_decode_bytes.restype = u64
    L.dtgpu_decode_last_ms.argtypes = [vp]
    L.dtgpu_decode_last_ms.restype = ctypes.c_float
    L.dtgpu_decode_free.argtypes = [vp]
    L.dtgpu_decode_profile.argtypes = [vp, sz, ctypes.POINTER(ctypes.c_uint32)]
    L.dtgpu_decode_add.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(sz), sz, c,
                                   ctypes.POINTER(ctypes.c_float), ctypes.POINTER(vp)]
    L.dtgpu_decode_add_result.argtypes = [vp, sz, pu64, sz, ctypes.POINTER(sz)]
    L.dtgpu_decode_history.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), pu64, ctypes.POINTER(sz), sz,
                                       ctypes.POINTER(ctypes.c_float), ctypes.POINTER(vp)]
    L.dtgpu_decode_history_result.argtypes = [vp, sz, pu64, sz, ctypes.POINTER(sz)]
    L.dtgpu_decode_encode_from.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), pu64, ctypes.POINTER(sz), sz,
                                           ctypes.c_uint32, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(vp)]
    L.dtgpu_patches_size.argtypes = [vp]
    L.dtgpu_patches_size.restype = sz
    L.dtgpu_patches_result.argtypes = [vp, sz, pu64, sz, ctypes.POINTER(sz)]
    L.dtgpu_patches_get.argtypes = [vp, sz, ctypes.c_char_p, sz, ctypes.POINTER(sz)]
    L.dtgpu_patches_profile.argtypes = [vp, sz, ctypes.POINTER(ctypes.c_uint32)]
    L.dtgpu_patches_free.argtypes = [vp]
    L.dtgpu_batch_create_decoded.argtypes = [vp, ctypes.POINTER(vp)]
    L.dtgpu_batch_create_decoded_opts.argtypes = [vp, ctypes.POINTER(BatchOpts), ctypes.POINTER(vp)]
    L.dtgpu_batch_blame.argtypes = [vp, sz, ctypes.POINTER(BlameRun), sz, ctypes.POINTER(sz)]
    L.dtgpu_batch_blame_agents.argtypes = [vp, sz, ctypes.c_char_p, sz, ctypes.POINTER(sz)]
    L.dtgpu_batch_blame_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    psz, pf, psum = ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(Summaries)
    L.dtgpu_oplog_summarize.argtypes = [vp, ctypes.c_char_p, sz, psz, psz, sz, pu64, sz, psz]
    L.dtgpu_oplog_intersect_summary.argtypes = [vp, psum, sz, pu64, sz, psz, pu64, sz, psz]
    L.dtgpu_decode_summarize.argtypes = [vp, sz, ctypes.c_char_p, sz, psz, psz, sz, pu64, sz, psz]
    L.dtgpu_decode_intersect.argtypes = [vp, psum, sz, pf, ctypes.POINTER(vp)]
    L.dtgpu_decode_encode_from_summaries.argtypes = [vp, psum, sz, ctypes.c_uint32, pf, ctypes.POINTER(vp),
                                                     ctypes.POINTER(vp)]
    L.dtgpu_intersect_size.argtypes = [vp]
    L.dtgpu_intersect_size.restype = sz
    L.dtgpu_intersect_result.argtypes = [vp, sz, pu64, sz, psz]
    L.dtgpu_intersect_remainder.argtypes = [vp, sz, pu64, sz, psz]
    L.dtgpu_intersect_profile.argtypes = [vp, sz, pu32]
    L.dtgpu_intersect_free.argtypes = [vp]
    L.dtgpu_decode_xf_from.argtypes = [vp, pu32, pu64, psz, pu64, psz, sz, pf, ctypes.POINTER(vp)]
    L.dtgpu_merges_size.argtypes = [vp]
    L.dtgpu_merges_size.restype = sz
    L.dtgpu_merges_result.argtypes = [vp, sz, pu64, sz, psz]
    L.dtgpu_merges_ops.argtypes = [vp, sz, pu32, sz, psz]
    L.dtgpu_merges_text.argtypes = [vp, sz, ctypes.c_char_p, sz, psz]
    L.dtgpu_merges_profile.argtypes = [vp, sz, pu32]
    L.dtgpu_merges_free.argtypes = [vp]
    L.dtgpu_graph_queries.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(sz), sz,
                                      ctypes.POINTER(GraphQuery), sz, ctypes.POINTER(ctypes.c_int64), sz,
                                      ctypes.POINTER(ctypes.c_int64), sz,
                                      ctypes.POINTER(GraphAnswer), ctypes.POINTER(ctypes.c_float)]
    L.dtgpu_status_str.argtypes = [c]
    L.dtgpu_status_str.restype = ctypes.c_char_p
    _lib = L
    return L


def _check(code):
    if code:
        raise ParseError(code)


def _u64s(xs):
    return (ctypes.c_uint64 * max(1, len(xs)))(*xs), len(xs)


def _csr(sets, n):
    """n sets of LVs flattened for the C ABI: (the u64 values, the n + 1 offsets)."""
    flat, off = [], [0]
    for v in sets:
        flat.extend(int(x) for x in v)
        off.append(len(flat))
    return _u64s(flat)[0], (ctypes.c_size_t * (n + 1))(*off)


def _sized(call, make):
    """The C ABI's sized read: call(None, 0, byref(n)) asks the length, call(buf, n, byref(n)) fills
    buf = make(n).  Returns (buf, n)."""
    n = ctypes.c_size_t()
    _check(call(None, 0, ctypes.byref(n)))
    buf = make(n.value)
    _check(call(buf, n.value, ctypes.byref(n)))
    return buf, n.value


def _sized_bytes(call) -> bytes:
    """_sized into a byte buffer: the bytes."""
    buf, n = _sized(call, lambda k: ctypes.create_string_buffer(max(1, k)))
    return buf.raw[:n]


def _frontier_result(fn, handle, i):
    """(status, frontier) of request i through a *_result call; a reduced frontier has at most 64 LVs."""
    k = ctypes.c_size_t()
    buf = (ctypes.c_uint64 * 64)()
    st = fn(handle, i, buf, 64, ctypes.byref(k))
    return st, list(buf[:k.value])


def _name_bytes(name) -> bytes:
    return bytes(name) if isinstance(name, (bytes, bytearray)) else str(name).encode()


def normalize_summary(summary):
    """A version summary as [(name bytes, [(start, end), ...])].  Accepts VersionSummary entries
    (name, ranges) and VersionSummaryFlat entries (name, next_seq), which stand for
    name: [(0, next_seq)] (src/causalgraph/summary.rs:13-30)."""
    out = []
    for name, x in summary:
        if isinstance(x, int):
            rs = [(0, x)] if x else []
        else:
            rs = [(int(a), int(b)) for a, b in x]
        out.append((_name_bytes(name), rs))
    return out


def summary_of_remote_frontier(rf):
    """A remote frontier [(name, seq)] as the summary of unit ranges name: [(seq, seq + 1)]."""
    return [(_name_bytes(name), [(int(q), int(q) + 1)]) for name, q in rf]


def _pack_summaries(summaries, docs=None, frontiers=None):
    """The flattened dtgpu_summaries of a list of normalized summaries; returns (struct, names per
    request).  The struct keeps its arrays alive."""
    n = len(summaries)
    entry_off, name_off, range_off, ranges, blob, names = [0], [0], [0], [], bytearray(), []
    for sm in summaries:
        names.append([nm for nm, _ in sm])
        for nm, rs in sm:
            blob += nm
            name_off.append(len(blob))
            for a, b in rs:
                ranges += [a, b]
            range_off.append(len(ranges) // 2)
        entry_off.append(len(name_off) - 1)
    S = Summaries()
    S._keep = [(ctypes.c_uint32 * max(n, 1))(*[int(d) for d in (docs if docs is not None else [0] * n)]),
               (ctypes.c_size_t * (n + 1))(*entry_off), bytes(blob),
               (ctypes.c_size_t * len(name_off))(*name_off), (ctypes.c_size_t * len(range_off))(*range_off),
               (ctypes.c_uint64 * max(1, len(ranges)))(*ranges)]
    S.doc, S.entry_off, S.names, S.name_off, S.range_off, S.ranges = S._keep
    if frontiers is not None:
        if len(frontiers) != n:
            raise ValueError("one frontier per summary")
        flat, off = [], [0]
        for f in frontiers:
            flat.extend(int(x) for x in f)
            off.append(len(flat))
        S._keep += [(ctypes.c_uint64 * max(1, len(flat)))(*flat), (ctypes.c_size_t * (n + 1))(*off)]
        S.versions, S.version_off = S._keep[-2:]
    return S, names


def _group_remainder(names, triples):
    """Remainder records (entry, start, end) -> [(name, [(start, end), ...])] as
    intersect_with_summary groups them (summary.rs:246-255): consecutive records of equal name
    merge into one entry.  No records: None."""
    out = []
    for e, a, b in triples:
        nm = names[e].decode(errors="surrogateescape")
        if out and out[-1][0] == nm:
            out[-1][1].append((a, b))
        else:
            out.append((nm, [(a, b)]))
    return out or None


def _read_summary(call):
    """dtgpu_oplog_summarize's query-size protocol -> [(name, [(start, end), ...])]."""
    sizes = (ctypes.c_size_t * 3)()
    _check(call(None, 0, None, None, 0, None, 0, sizes))
    ne, nb, nr = sizes[0], sizes[1], sizes[2]
    names = ctypes.create_string_buffer(max(1, nb))
    name_off, range_off = (ctypes.c_size_t * (ne + 1))(), (ctypes.c_size_t * (ne + 1))()
    ranges = (ctypes.c_uint64 * max(1, 2 * nr))()
    _check(call(names, nb, name_off, range_off, ne, ranges, nr, sizes))
    return [(names.raw[name_off[e]:name_off[e + 1]].decode(errors="surrogateescape"),
             [(ranges[2 * k], ranges[2 * k + 1]) for k in range(range_off[e], range_off[e + 1])]) for e in range(ne)]


def merge_xf_runs(ops, content, char_offsets, stream):
    """The run-merging of iter_xf_operations over a decoded oplog's arrays (`ops` as export("ops"),
    the inserted `content` bytes, the per-LV `char_offsets`) and a stream of (lv, pos | None) in
    application order: yields (range(lv, lv+len), op).  Consecutive LVs of one op run are merged
    when they form one reference-style op: an insert at consecutive positions, a forward delete at
    one position, a backspace run at descending positions (reported at its lowest position, like
    BaseMoved)."""
    ops = ops.reshape(-1, 4)
    coff = char_offsets
    run_of = {}
    for r, (lv, ln, _pos, kf) in enumerate(ops):
        for k in range(int(ln)):
            run_of[int(lv) + k] = (r, int(kf) & 1)

    def char(v):
        b = coff[v]
        n = 1 if content[b] < 0x80 else 2 if content[b] < 0xE0 else 3 if content[b] < 0xF0 else 4
        return content[b:b + n].decode("utf-8")

    cur = None   # [start_lv, end_lv, run, kind, first_pos, last_pos, text, step]
    for lv, x in stream:
        r, kind = run_of[lv]
        if cur is not None and lv == cur[1] and r == cur[2]:
            if x is None and cur[3] is None:
                cur[1] += 1
                continue
            if x is not None and cur[3] == kind:
                step = x - cur[5]
                want = {0: (1,), 1: (0, -1)}[kind] if cur[7] is None else (cur[7],)
                if step in want and (kind == 0 or cur[1] - cur[0] == 1 or step == cur[7]):
                    cur[1] += 1
                    cur[5] = x
                    cur[7] = step
                    if kind == 0:
                        cur[6] += char(lv)
                    continue
        if cur is not None:
            yield _xf_item(cur)
        cur = [lv, lv + 1, r, None if x is None else kind, x, x, char(lv) if (x is not None and kind == 0) else "", None]
    if cur is not None:
        yield _xf_item(cur)


def _xf_item(cur):
    rng = range(cur[0], cur[1])
    if cur[3] is None:
        return rng, None
    if cur[3] == 0:
        return rng, ("ins", cur[4], cur[6])
    return rng, ("del", min(cur[4], cur[5]), cur[1] - cur[0])


def text_hash(data: bytes) -> int:
    return lib().dtgpu_text_hash(data, len(data))


class ListBranch:
    """Result of a checkout: `ListBranch` (src/list/mod.rs:65-76) content + version."""

    def __init__(self, content: bytes = b"", version=()):
        self._content = content
        self.version = list(version)

    @classmethod
    def new(cls) -> "ListBranch":
        """ListBranch::new() (src/list/branch.rs:12-20): empty content at ROOT."""
        return cls()

    @classmethod
    def new_at_local_version(cls, oplog: "ListOpLog", version) -> "ListBranch":
        """ListBranch::new_at_local_version (src/list/branch.rs:22-26) = oplog.checkout(version)."""
        return oplog.checkout(version)

    @classmethod
    def new_at_tip(cls, oplog: "ListOpLog") -> "ListBranch":
        """ListBranch::new_at_tip (src/list/branch.rs:30-32)."""
        return oplog.checkout_tip()

    def merge(self, oplog: "ListOpLog", merge_frontier) -> None:
        """ListBranch::merge(&mut self, oplog, merge_frontier) (src/list/merge.rs:63-95): apply
        the transformed operations iter_xf_operations_from(self.version, merge_frontier)
        (computed on the GPU) to this branch's content, then move to
        find_dominators_2(self.version, merge_frontier)."""
        v = oplog.dominators(self.version, merge_frontier)
        if v == self.version:
            return
        text = list(self.content())
        for _rng, op in oplog.iter_xf_operations(self.version, merge_frontier):
            if op is None:
                continue
            if op[0] == "ins":
                text[op[1]:op[1]] = list(op[2])
            else:
                del text[op[1]:op[1] + op[2]]
        self._content = "".join(text).encode()
        self.version = v

    def content(self) -> str:
        return self._content.decode("utf-8")

    def content_bytes(self) -> bytes:
        return self._content

    def __len__(self):
        return len(self.content())

    def len(self):
        return len(self)

    def local_frontier(self):
        return list(self.version)


class EncodeOptions(collections.namedtuple(
        "EncodeOptions", "store_inserted_content compress_content store_start_branch_content")):
    """EncodeOptions (src/list/encoding/encode_oplog.rs:88-110): the fields libdtgpu honours
    (user_data, store_deleted_content and the experimental end branch are not offered)."""
    def flags(self):
        return ((1 if self.store_inserted_content else 0) | (2 if self.compress_content else 0)
                | (4 if self.store_start_branch_content else 0))


ENCODE_FULL = EncodeOptions(True, True, True)     # encode_oplog.rs:122-130
ENCODE_PATCH = EncodeOptions(True, True, False)   # encode_oplog.rs:112-120


def lz4_compress(data: bytes) -> bytes:
    """lz4_flex::compress_into as the encoder calls it (encode_oplog.rs:320-343): one raw LZ4
    block, no length prefix."""
    return _sized_bytes(lambda *a: lib().dtgpu_lz4_compress(data, len(data), *a))


class ListOpLog:
    """Mirror of `ListOpLog` (src/list/mod.rs:103-126) for the checkout path."""

    def __init__(self, _handle=None):
        self._h = _handle if _handle is not None else lib().dtgpu_oplog_new()

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib().dtgpu_oplog_free(h)
            self._h = None

    @classmethod
    def load_from(cls, data: bytes, ignore_crc: bool = False) -> "ListOpLog":
        out = ctypes.c_void_p()
        _check(lib().dtgpu_oplog_load(data, len(data), int(ignore_crc), ctypes.byref(out)))
        return cls(out.value)

    def decode_and_add(self, data: bytes, ignore_crc: bool = False):
        """ListOpLog::decode_and_add(_opts) (src/list/encoding/decode_oplog.rs:465-583): merge a
        `.dt` file or patch, skipping operations already here; returns the file's version.  On a
        ParseError the oplog is left as it was."""
        cap = 64
        buf = (ctypes.c_uint64 * cap)()
        n = ctypes.c_size_t()
        _check(lib().dtgpu_oplog_decode_and_add(self._h, data, len(data), int(ignore_crc), buf, cap, ctypes.byref(n)))
        if n.value <= cap:
            return list(buf[:n.value])
        # a wider version than the buffer: read the reported frontier back (adds nothing)
        full = (ctypes.c_uint64 * n.value)()
        lib().dtgpu_oplog_last_added_frontier(self._h, full, n.value)
        return list(full)

    @property
    def doc_id(self):
        """ListOpLog::doc_id (src/list/mod.rs:109): None or the document id string."""
        n = lib().dtgpu_oplog_doc_id(self._h, None, 0)
        if n < 0:
            return None
        buf = ctypes.create_string_buffer(max(1, n))
        lib().dtgpu_oplog_doc_id(self._h, buf, n)
        return buf.raw[:n].decode()

    @doc_id.setter
    def doc_id(self, value):
        if value is None:
            _check(lib().dtgpu_oplog_set_doc_id(self._h, None, 0))
        else:
            b = value.encode()
            _check(lib().dtgpu_oplog_set_doc_id(self._h, b, len(b)))

    def __len__(self):
        return lib().dtgpu_oplog_len(self._h)

    def get_or_create_agent_id(self, name: str) -> int:
        b = name.encode()
        a = lib().dtgpu_oplog_get_or_create_agent_id(self._h, b, len(b))
        if a < 0:
            raise ValueError(f"invalid agent name {name!r}")
        return a

    def add_insert_at(self, agent: int, parents, pos: int, content: str) -> int:
        p, n = _u64s(parents)
        b = content.encode()
        return lib().dtgpu_oplog_add_insert_at(self._h, agent, p, n, pos, b, len(b))

    def add_delete_at(self, agent: int, parents, start: int, end: int) -> int:
        p, n = _u64s(parents)
        return lib().dtgpu_oplog_add_delete_at(self._h, agent, p, n, start, end)

    def add_insert(self, agent: int, pos: int, content: str) -> int:
        b = content.encode()
        return lib().dtgpu_oplog_add_insert(self._h, agent, pos, b, len(b))

    def add_delete_without_content(self, agent: int, start: int, end: int) -> int:
        return lib().dtgpu_oplog_add_delete_without_content(self._h, agent, start, end)

    def local_frontier(self):
        buf = (ctypes.c_uint64 * 64)()
        n = lib().dtgpu_oplog_local_frontier(self._h, buf, 64)
        if n > 64:
            buf = (ctypes.c_uint64 * n)()
            lib().dtgpu_oplog_local_frontier(self._h, buf, n)
        return list(buf[:n])

    def plan_stats(self):
        out = (ctypes.c_uint64 * 4)()
        _check(lib().dtgpu_oplog_plan_stats(self._h, out))
        return dict(steps=out[0], retreat=out[1], advance=out[2], commands=out[3])

    def plan_commands(self):
        n = lib().dtgpu_oplog_plan_commands(self._h, None, 0)
        buf = (ctypes.c_uint32 * max(4, 4 * n))()
        lib().dtgpu_oplog_plan_commands(self._h, buf, n)
        return [tuple(buf[4 * i:4 * i + 4]) for i in range(n)]

    def plan_tlist(self):
        n = lib().dtgpu_oplog_plan_tlist(self._h, None, 0)
        buf = (ctypes.c_uint32 * max(1, n))()
        lib().dtgpu_oplog_plan_tlist(self._h, buf, n)
        return list(buf[:n])

    def ins_content(self) -> bytes:
        n = lib().dtgpu_oplog_ins_content(self._h, None, 0)
        buf = ctypes.create_string_buffer(max(1, n))
        lib().dtgpu_oplog_ins_content(self._h, buf, n)
        return buf.raw[:n]

    def char_offsets(self):
        n = lib().dtgpu_oplog_char_offsets(self._h, None, 0)
        buf = (ctypes.c_uint32 * max(1, n))()
        lib().dtgpu_oplog_char_offsets(self._h, buf, n)
        return list(buf[:n])

    def agent_runs(self):
        n = lib().dtgpu_oplog_agent_runs(self._h, None, 0)
        buf = (ctypes.c_uint32 * max(1, n))()
        lib().dtgpu_oplog_agent_runs(self._h, buf, n)
        return list(buf[:n])

    def export(self, what):
        """The decoded oplog's arrays (dtgpu_oplog_export): "ops", "agent_runs", "entries",
        "parent_offsets", "parents", "content", "char_offsets", "version", "agent_names"."""
        a = _export(lambda c, p, n: lib().dtgpu_oplog_export(self._h, c, p, n), what)
        return _names(a) if what == "agent_names" else a

    def cut_ranges(self):
        """Maximal [first, last] LV ranges of cut points (dtgpu_oplog_cut_ranges): v such that the
        ops below v are the version {v-1} and every later op has v-1 in its history."""
        n = lib().dtgpu_oplog_cut_ranges(self._h, None, 0)
        buf = (ctypes.c_uint64 * max(2, 2 * n))()
        lib().dtgpu_oplog_cut_ranges(self._h, buf, n)
        return [(int(buf[2 * k]), int(buf[2 * k + 1])) for k in range(n)]

    def checkout_tip_bytes(self) -> bytes:
        return _sized_bytes(lambda *a: lib().dtgpu_checkout_tip(self._h, *a))

    def checkout_tip(self) -> ListBranch:
        return ListBranch(self.checkout_tip_bytes(), self.local_frontier())

    def xf_order(self, frm=None, merging=None):
        """LV order of iter_xf_operations(_from) (host plan: fast-forward prefix, then the
        walker); default ROOT to the tip."""
        if frm is None and merging is None:
            frm, merging = [], self.local_frontier()
        pa, na = _u64s(frm or [])
        pb, nb = _u64s(merging or [])
        n = len(self)
        buf = (ctypes.c_uint32 * max(1, n))()
        k = lib().dtgpu_oplog_xf_order(self._h, pa, na, pb, nb, buf, n)
        return list(buf[:k])

    def xf_operations_lv(self, frm=None, merging=None):
        """Per-LV transformed positions in application order, computed on the GPU
        (dtgpu_xf_operations_from; default: ROOT to the tip): [(lv, pos or None)], None =
        DeleteAlreadyHappened."""
        if frm is None and merging is None:
            frm, merging = [], self.local_frontier()
        pa, na = _u64s(frm or [])
        pb, nb = _u64s(merging or [])
        buf, n = _sized(lambda *a: lib().dtgpu_xf_operations_from(self._h, pa, na, pb, nb, *a),
                        lambda k: (ctypes.c_uint32 * max(2, 2 * k))())
        return [(buf[2 * i], None if buf[2 * i + 1] == 0xFFFFFFFF else buf[2 * i + 1]) for i in range(n)]

    def iter_xf_operations_from(self, frm, merging):
        """ListOpLog::iter_xf_operations_from (src/list/merge.rs:24-38); see iter_xf_operations."""
        return self.iter_xf_operations(frm, merging)

    def iter_xf_operations(self, frm=None, merging=None):
        """ListOpLog::iter_xf_operations() (src/list/merge.rs:40-48): yields (range(lv, lv+len),
        op) with op = ("ins", pos, text) / ("del", pos, len) / None (DeleteAlreadyHappened).
        Consecutive LVs of one op run are merged when they form one reference-style op
        (merge_xf_runs)."""
        return merge_xf_runs(self.export("ops"), self.ins_content(), self.char_offsets(),
                             self.xf_operations_lv(frm, merging))

    def encode(self, opts=None) -> bytes:
        """ListOpLog::encode(opts) (src/list/encoding/encode_oplog.rs:745-747); opts defaults to
        ENCODE_FULL (EncodeOptions::default, :133-137)."""
        return self.encode_from([], opts)

    def encode_from(self, frm, opts=None) -> bytes:
        """ListOpLog::encode_from(opts, from) (encode_oplog.rs:404-743): the ops after version
        `frm`.  With opts.store_start_branch_content and a non-ROOT `frm`, the StartBranch holds
        the checkout at `frm`, run on the GPU."""
        p, nf = _u64s(frm)
        flags = (opts or ENCODE_FULL).flags()
        return _sized_bytes(lambda *a: lib().dtgpu_oplog_encode(self._h, p, nf, flags, *a))

    def dominators(self, a, b=()):
        """Graph::find_dominators_2 (src/causalgraph/graph/tools.rs:545-578) over this oplog."""
        pa, na = _u64s(a)
        pb, nb = _u64s(b)
        cap = na + nb + 1
        out = (ctypes.c_uint64 * cap)()
        n = lib().dtgpu_oplog_dominators(self._h, pa, na, pb, nb, out, cap)
        if n < 0:
            raise ValueError("version names an LV outside the oplog")
        return list(out[:n])

    def checkout_bytes(self, version) -> bytes:
        p, nv = _u64s(version)
        return _sized_bytes(lambda *a: lib().dtgpu_checkout(self._h, p, nv, *a))

    def history(self, version) -> "ListOpLog":
        """The history of `version` as its own oplog (dtgpu_oplog_history)."""
        p, nv = _u64s(version)
        out = ctypes.c_void_p()
        _check(lib().dtgpu_oplog_history(self._h, p, nv, ctypes.byref(out)))
        return ListOpLog(out.value)

    def project(self, spans) -> "ListOpLog":
        """The ops in the LV spans [(start, end), ...] with the causal graph projected onto them
        (Graph::subgraph_raw, src/causalgraph/graph/subgraph.rs:39-250; dtgpu_oplog_project)."""
        flat = [int(x) for s in spans for x in s]
        p = (ctypes.c_uint64 * max(1, len(flat)))(*flat)
        out = ctypes.c_void_p()
        _check(lib().dtgpu_oplog_project(self._h, p, len(flat) // 2, ctypes.byref(out)))
        return ListOpLog(out.value)

    def project_version(self, spans, version):
        """A version of this oplog projected onto the sub-oplog of `spans` (the numbering
        `project(spans)` gives): the frontier of Hist(version) n spans
        (Graph::project_onto_subgraph_raw; dtgpu_oplog_project_version)."""
        flat = [int(x) for s in spans for x in s]
        p = (ctypes.c_uint64 * max(1, len(flat)))(*flat)
        pv, nv = _u64s(version)
        cap = max(1, len(flat))
        out = (ctypes.c_uint64 * cap)()
        n = lib().dtgpu_oplog_project_version(self._h, p, len(flat) // 2, pv, nv, out, cap)
        if n < 0:
            raise ValueError("bad spans or version")
        if n > cap:
            out = (ctypes.c_uint64 * n)()
            n = lib().dtgpu_oplog_project_version(self._h, p, len(flat) // 2, pv, nv, out, n)
        return list(out[:n])

    def local_to_remote(self, lv):
        """AgentAssignment::local_to_agent_version: LV -> (agent id, seq)."""
        a, q = ctypes.c_uint32(), ctypes.c_uint64()
        _check(lib().dtgpu_oplog_local_to_remote(self._h, lv, ctypes.byref(a), ctypes.byref(q)))
        return a.value, q.value

    def remote_to_local(self, agent, seq, n=1):
        """Local LV spans [(start, end)] of the remote span (agent id, seq .. seq + n), in seq
        order; KeyError when part of it is unknown here."""
        cap = 8
        while True:
            buf = (ctypes.c_uint64 * (2 * cap))()
            k = lib().dtgpu_oplog_remote_to_local(self._h, agent, seq, n, buf, cap)
            if k < 0:
                raise KeyError((agent, seq, n))
            if k <= cap:
                return [(buf[2 * i], buf[2 * i + 1]) for i in range(k)]
            cap = k

    def summarize_versions(self):
        """AgentAssignment::summarize_versions (src/causalgraph/summary.rs:119-132):
        [(name, [(seq start, seq end), ...])] per agent with ops, in agent-id order."""
        return _read_summary(lambda *a: lib().dtgpu_oplog_summarize(self._h, *a))

    def intersect_with_summary(self, summary, frontier=()):
        """CausalGraph::intersect_with_summary (src/causalgraph/summary.rs:234-264): (the version the
        summary's owner and this oplog share, as a frontier of local LVs; what the owner has and
        this oplog lacks as [(name, ranges)], or None).  `summary` may be flat, [(name, next_seq)]."""
        st, f, triples = self.intersect_summary_records(summary, frontier)
        _check(st)
        return f, _group_remainder([nm for nm, _ in normalize_summary(summary)], triples)

    def intersect_summary_records(self, summary, frontier=()):
        """dtgpu_oplog_intersect_summary as it is: (status, frontier, remainder records (entry index,
        start, end)) -- what the batched device call is compared with, request for request."""
        S, _ = _pack_summaries([normalize_summary(summary)], frontiers=[list(frontier)])
        nf, nt = ctypes.c_size_t(), ctypes.c_size_t()
        st = lib().dtgpu_oplog_intersect_summary(self._h, ctypes.byref(S), 0, None, 0, ctypes.byref(nf), None, 0,
                                                 ctypes.byref(nt))
        if st:
            return st, [], []
        f, t = (ctypes.c_uint64 * max(1, nf.value))(), (ctypes.c_uint64 * max(1, 3 * nt.value))()
        st = lib().dtgpu_oplog_intersect_summary(self._h, ctypes.byref(S), 0, f, nf.value, ctypes.byref(nf), t,
                                                 nt.value, ctypes.byref(nt))
        return st, list(f[:nf.value]), [(t[3 * k], t[3 * k + 1], t[3 * k + 2]) for k in range(nt.value)]

    def remote_frontier_to_local(self, rf, frontier=()):
        """A remote frontier [(name, seq)] as a frontier of local LVs; KeyError when this oplog
        lacks one of those versions."""
        f, rem = self.intersect_with_summary(summary_of_remote_frontier(rf), frontier)
        if rem is not None:
            raise KeyError(rem)
        return f

    def checkout_text_bytes(self, spans) -> bytes:
        """OpLog::checkout_text (src/oplog.rs:388-394) for the text whose ops are `spans`: the
        projected sub-oplog checked out on the device."""
        return self.project(spans).checkout_tip_bytes()

    def checkout(self, version) -> ListBranch:
        """ListOpLog::checkout(&[LV]) (src/list/oplog.rs:32-36): the branch at `version`."""
        v = self.dominators(version)
        return ListBranch(self.checkout_bytes(v), v)

    def blame(self, version=None):
        """Who wrote each character of the text at `version` (default: the tip), as
        Batch.blame_spans gives it: [(agent_name, seq_start, seq_end, char_start, char_end)] in text
        order.  At a version the history is projected first (history), which renumbers LVs; the
        (agent name, seq) spans hold across numberings."""
        if version is not None and not len(version):
            return []
        o = self if version is None else self.history(version)
        b = Batch(oplogs=[o], blame=True)
        b.run()
        b.sync()
        _check(b.results()[0]["status"])
        return b.blame_spans(0)


# dtgpu_export codes (include/dtgpu.h): name -> (code, numpy dtype, fields per record)
EXPORTS = {
    "ops": (0, "<u4", 4), "agent_runs": (1, "<u4", 4), "entries": (2, "<u4", 2),
    "parent_offsets": (3, "<u4", 1), "parents": (4, "<u4", 1), "content": (5, "u1", 1),
    "char_offsets": (6, "<u4", 1), "version": (7, "<u4", 1), "agent_names": (8, "u1", 1),
    "doc_id": (9, "u1", 1),
}
DECODE_DEFER = 80


def _export(fn, what):
    import numpy as np
    code, dt, per = EXPORTS[what]
    n = fn(code, None, 0)
    arr = np.zeros(max(n, 1) * per, dtype=dt)
    fn(code, arr.ctypes.data_as(ctypes.c_void_p), n)
    arr = arr[:n * per]
    return arr.reshape(n, per) if per > 1 else arr


def _names(blob):
    out, i = [], 0
    blob = bytes(blob)
    while i < len(blob):
        k = blob[i]
        out.append(blob[i + 1:i + 1 + k])
        i += 1 + k
    return out


def oplog_from_trace(txns, agent_name="jeremy") -> ListOpLog:
    """crates/bench/src/utils.rs:25-44 apply_edits_push_merge (delete then insert per patch)."""
    o = ListOpLog()
    a = o.get_or_create_agent_id(agent_name)
    for txn in txns:
        for pos, dl, ins in txn["patches"]:
            if dl > 0:
                o.add_delete_without_content(a, pos, pos + dl)
            if ins:
                o.add_insert(a, pos, ins)
    return o


class Batch:
    """A batch staged in HBM.  staging="host": decode and planner inputs on host threads;
    staging="device": `.dt` bytes to HBM, then decode (dt_decode.hip) and planner inputs
    (dt_prep.hip) on the GPU as well.  Walk planning (dt_plan.hip), replay and materialisation
    (dt_replay.hip) always run on the GPU."""

    def __init__(self, docs=None, oplogs=None, ignore_crc=False, host_threads=0, device=0, staging="host",
                 xf=False, flags=0, seg_ops=0, seg_max=0, lds_fill=0, blame=False):
        """xf=True (with oplogs): a transformed-ops batch, every document's iter_xf_operations()
        computed by the replay (dtgpu_batch_create_xf); read it with xf_positions(i).  flags
        (OPT_*), seg_ops, seg_max, lds_fill: dtgpu_batch_opts.  blame=True (OPT_BLAME; not with
        xf): every run also leaves each document's blame, read with blame(i) / blame_spans(i)."""
        L = lib()
        if blame:
            flags = int(flags) | OPT_BLAME
        opts = BatchOpts(int(ignore_crc), int(host_threads), int(device), int(flags), int(seg_ops), int(seg_max),
                         int(lds_fill))
        out = ctypes.c_void_p()
        if oplogs is not None:
            arr = (ctypes.c_void_p * max(1, len(oplogs)))(*[o._h for o in oplogs])
            self._keep = oplogs
            create = L.dtgpu_batch_create_xf if xf else L.dtgpu_batch_create_from_oplogs
            _check(create(arr, len(oplogs), ctypes.byref(opts), ctypes.byref(out)))
            self.n = len(oplogs)
        else:
            self._keep = list(docs)
            ptrs = (ctypes.c_char_p * max(1, len(self._keep)))(*self._keep)
            lens = (ctypes.c_size_t * max(1, len(self._keep)))(*[len(d) for d in self._keep])
            create = L.dtgpu_batch_create_device if staging == "device" else L.dtgpu_batch_create
            _check(create(ptrs, lens, len(self._keep), ctypes.byref(opts), ctypes.byref(out)))
            self.n = len(self._keep)
        self._h = out.value

    def __len__(self):
        return self.n

    def xf_positions(self, i):
        """Per-LV BaseMoved positions of document i (xf batches; None = DeleteAlreadyHappened)."""
        buf, n = _sized(lambda *a: lib().dtgpu_batch_xf_positions(self._h, i, *a), lambda k: (ctypes.c_uint32 * max(1, k))())
        return [None if x == 0xFFFFFFFF else x for x in buf[:n]]

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib().dtgpu_batch_free(h)
            self._h = None

    def run(self, stream=None):
        _check(lib().dtgpu_batch_run(self._h, stream))

    def run_timed(self) -> float:
        ms = ctypes.c_float()
        _check(lib().dtgpu_batch_run_timed(self._h, ctypes.byref(ms)))
        return ms.value

    def run_e2e_timed(self):
        """Device-staged batches: decode + prep + plan + replay again; kernel ms of each."""
        ms = (ctypes.c_float * 4)()
        _check(lib().dtgpu_batch_run_e2e_timed(self._h, ms))
        return list(ms)

    def encode(self, opts=None) -> float:
        """Device-staged batches: ListOpLog::encode(opts) from ROOT for every document on the GPU
        (dtgpu_batch_encode); returns the encode kernel's ms.  Read the bytes with encoded(i)."""
        ms = ctypes.c_float()
        _check(lib().dtgpu_batch_encode(self._h, (opts or ENCODE_FULL).flags(), ctypes.byref(ms)))
        return ms.value

    def encoded(self, i) -> bytes:
        return _sized_bytes(lambda *a: lib().dtgpu_batch_encoded(self._h, i, *a, None))

    def encoded_status(self, i) -> int:
        n = ctypes.c_size_t()
        return lib().dtgpu_batch_encoded(self._h, i, None, 0, ctypes.byref(n), None)

    def encode_profile(self, i):
        n = ctypes.c_size_t()
        out = (ctypes.c_uint64 * 14)()
        _check(lib().dtgpu_batch_encoded(self._h, i, None, 0, ctypes.byref(n), out))
        return dict(zip(["walk", "op_runs", "sizes", "text_lz4", "write", "crc", "lz_probe", "lz_extend",
                         "lz_emit", "lz_steps", "lz_shared_steps", "lz_sequences", "txn_heads", "agent_runs"], list(out)))

    def encoded_bytes(self, which=0) -> int:
        return lib().dtgpu_batch_encoded_bytes(self._h, which)

    def sync(self):
        _check(lib().dtgpu_batch_sync(self._h))

    def results(self):
        arr = (DocResult * max(1, self.n))()
        _check(lib().dtgpu_batch_results(self._h, arr))
        return [dict(status=r.status, text_len=r.text_len, text_hash=r.text_hash, n_lv=r.n_lv) for r in arr[:self.n]]

    def text(self, i) -> bytes:
        return _sized_bytes(lambda *a: lib().dtgpu_batch_text(self._h, i, *a))

    def blame(self, i):
        """Blame batches: document i's text as maximal runs [(lv, len, agent, seq)] in text order
        (dtgpu_batch_blame): `len` characters, character k inserted by LV lv + k = (agent, seq + k).
        A document that failed raises ParseError with its status."""
        buf, n = _sized(lambda *a: lib().dtgpu_batch_blame(self._h, i, *a), lambda k: (BlameRun * max(1, k))())
        return [(r.lv, r.len, r.agent, r.seq) for r in buf[:n]]

    def blame_agents(self, i):
        """The names (bytes) of document i's agent ids, indexed by a run's agent."""
        return _names(_sized_bytes(lambda *a: lib().dtgpu_batch_blame_agents(self._h, i, *a)))

    def blame_spans(self, i):
        """blame(i) by name: [(agent_name, seq_start, seq_end, char_start, char_end)], the characters
        text(i).decode()[char_start:char_end] being (agent_name, seq_start .. seq_end - 1).  Adjacent
        runs of one agent whose seqs continue are one span even where their LVs do not (LVs are
        local to an oplog: a merge or a projection numbers them anew), so the spans of a text are
        the same under every numbering."""
        names = self.blame_agents(i)
        out, at = [], 0
        for _, n, agent, seq in self.blame(i):
            if out and out[-1][0] == names[agent] and out[-1][2] == seq:
                out[-1] = out[-1][:2] + (seq + n, out[-1][3], at + n)
            else:
                out.append((names[agent], seq, seq + n, at, at + n))
            at += n
        return out

    def blame_stats(self):
        """Of the last run (dtgpu_batch_blame_stats): runs, characters, the blame kernels' us, bytes
        of the source-list and run arenas."""
        out = (ctypes.c_uint64 * 4)()
        _check(lib().dtgpu_batch_blame_stats(self._h, out))
        return dict(zip(["runs", "chars", "kernel_us", "arena_bytes"], [int(x) for x in out]))

    def last_times(self):
        """(plan_ms, replay_ms, prep_ms) of the last run_timed() (prep_ms 0 when host-staged)."""
        out = (ctypes.c_float * 3)()
        _check(lib().dtgpu_batch_last_times(self._h, out))
        return out[0], out[1], out[2]

    def host_planned(self):
        n = len(self)
        buf = (ctypes.c_uint8 * max(1, n))()
        lib().dtgpu_batch_host_planned(self._h, buf, n)
        return [int(x) for x in buf[:n]]

    def fast_forwarded(self):
        """Per document: 1 when it checked out on the fast-forward path (dt_ff.hip: a linear
        history, merge.rs:811-840), else 0."""
        n = len(self)
        buf = (ctypes.c_uint8 * max(1, n))()
        lib().dtgpu_batch_fast_forwarded(self._h, buf, n)
        return [int(x) for x in buf[:n]]

    def late_pipelined(self):
        """Per document: 1 when every pass runs it in the late pipeline (dtgpu_batch_late_pipelined),
        else 0; all 0 when the batch runs one pipeline."""
        n = len(self)
        buf = (ctypes.c_uint8 * max(1, n))()
        lib().dtgpu_batch_late_pipelined(self._h, buf, n)
        return [int(x) for x in buf[:n]]

    def plan(self, i):
        """Command stream (op, lv, len, pos) and retreat/advance entries of document i."""
        nc, nt = ctypes.c_size_t(), ctypes.c_size_t()
        _check(lib().dtgpu_batch_plan(self._h, i, None, 0, None, 0, ctypes.byref(nc), ctypes.byref(nt)))
        cb = (ctypes.c_uint32 * max(4, 4 * nc.value))()
        tb = (ctypes.c_uint32 * max(1, nt.value))()
        _check(lib().dtgpu_batch_plan(self._h, i, cb, nc.value, tb, nt.value, ctypes.byref(nc), ctypes.byref(nt)))
        return [tuple(cb[4 * k:4 * k + 4]) for k in range(nc.value)], list(tb[:nt.value])

    def plan_profile(self, i):
        out = (ctypes.c_uint64 * 8)()
        _check(lib().dtgpu_batch_plan_profile(self._h, i, out))
        keys = ["rec", "parents", "children", "emit", "ops", "init", "n_cmds", "n_tlist"]
        return dict(zip(keys, list(out)))

    def doc_stats(self, i):
        """Diagnostics of document i after a run (see dtgpu_batch_doc_stats)."""
        out = (ctypes.c_uint32 * 29)()
        _check(lib().dtgpu_batch_doc_stats(self._h, i, out))
        keys = ["n_items", "n_blocks", "fail_cmd", "fail_site", "n_cmds", "max_blocks",
                "cyc_ins", "cyc_del", "cyc_tog", "cyc_mat", "cyc_yjs", "cyc_split", "cyc_find", "cyc_bload",
                "cyc_orr", "cyc_run", "cyc_r1", "cyc_r2", "cyc_r3", "n_yjs", "n_split", "cyc_total",
                "n_sb", "lds_index", "cyc_t1", "cyc_t2", "cyc_t3", "n_dirty", "n_load"]
        st = dict(zip(keys, list(out)))
        look = (ctypes.c_uint32 * 2)()   # position lookups, and those the cached block answered
        _check(lib().dtgpu_batch_lookup_stats(self._h, i, look))
        st["n_lookup"], st["n_lookup_skip"] = look[0], look[1]
        return st

    def segments(self, i):
        """Cut replay: the LV segments document i replayed as (see dtgpu_batch_segments), as
        dicts; [] when it replayed whole."""
        out = (ctypes.c_uint32 * (12 * 64))()
        n = lib().dtgpu_batch_segments(self._h, i, out, 64)
        keys = ["lo", "hi", "placeholders", "status", "items_visible", "cyc_total", "lds_index", "n_blocks",
                "host_fallback", "host_lo", "host_hi", "host_placeholders"]
        return [dict(zip(keys, list(out[12 * k:12 * k + 12]))) for k in range(min(n, 64))]

    @property
    def algorithmic_bytes(self):
        return lib().dtgpu_batch_algorithmic_bytes(self._h)

    @property
    def total_lv(self):
        return lib().dtgpu_batch_total_lv(self._h)


class DecodeBatch:
    """Batched `ListOpLog::load_from` on the GPU (dtgpu_decode_*): one wavefront per document."""

    def __init__(self, docs, ignore_crc=False, device=0):
        L = lib()
        n = len(docs)
        self._keep = [bytes(d) for d in docs]
        arr = (ctypes.c_char_p * max(n, 1))(*self._keep)
        lens = (ctypes.c_size_t * max(n, 1))(*[len(d) for d in self._keep])
        opts = BatchOpts(1 if ignore_crc else 0, 0, device)
        h = ctypes.c_void_p()
        _check(L.dtgpu_decode_create(arr, lens, n, ctypes.byref(opts), ctypes.byref(h)))
        self._h = h
        self.n = n

    def __len__(self):
        return self.n

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib().dtgpu_decode_free(h)
            self._h = None

    def run(self) -> float:
        """Full device decode of every document; returns the kernel time in ms."""
        ms = ctypes.c_float()
        _check(lib().dtgpu_decode_run(self._h, ctypes.byref(ms)))
        return ms.value

    def status(self, i):
        out = (ctypes.c_uint64 * 12)()
        _check(lib().dtgpu_decode_status(self._h, i, out))
        keys = ("status", "n_lv", "n_ops", "n_aruns", "n_entries", "n_parents", "n_content", "n_version",
                "n_agents", "content_complete", "ascii", "n_file_agents")
        return dict(zip(keys, list(out)))

    def export(self, i, what):
        a = _export(lambda c, p, n: lib().dtgpu_decode_export(self._h, i, c, p, n), what)
        return _names(a) if what == "agent_names" else a

    def doc_id(self, i):
        a = bytes(self.export(i, "doc_id"))
        return a[1:].decode() if a and a[0] else None

    def add(self, patches, ignore_crc=False):
        """ListOpLog::decode_and_add of patches[i] into document i, on the GPU (dtgpu_decode_add):
        a new DecodeBatch of the merged oplogs (this one is unchanged).  Per-document outcome:
        add_result(i)."""
        n = len(patches)
        keep = [bytes(p) for p in patches]
        arr = (ctypes.c_char_p * max(n, 1))(*keep)
        lens = (ctypes.c_size_t * max(n, 1))(*[len(p) for p in keep])
        ms = ctypes.c_float()
        h = ctypes.c_void_p()
        _check(lib().dtgpu_decode_add(self._h, arr, lens, n, int(ignore_crc), ctypes.byref(ms), ctypes.byref(h)))
        m = DecodeBatch.__new__(DecodeBatch)
        m._h, m.n, m._keep, m.last_ms = h, n, keep, ms.value
        return m

    def add_result(self, i):
        """(status, the patch's version): decode_and_add's Result for document i of a merged batch."""
        return _frontier_result(lib().dtgpu_decode_add_result, self._h, i)

    def history(self, docs, versions):
        """ListOpLog::checkout(&[LV]) up to the replay, batched on the GPU (dtgpu_decode_history):
        a new DecodeBatch whose oplog i is the history of versions[i] (any set of LVs; [] is ROOT)
        of document docs[i] of this one (unchanged).  Per-output outcome: history_result(i)."""
        n = len(docs)
        if len(versions) != n:
            raise ValueError("one version per document index")
        d = (ctypes.c_uint32 * max(n, 1))(*[int(x) for x in docs])
        pv, po = _csr(versions, n)
        ms = ctypes.c_float()
        h = ctypes.c_void_p()
        _check(lib().dtgpu_decode_history(self._h, d, pv, po, n, ctypes.byref(ms), ctypes.byref(h)))
        m = DecodeBatch.__new__(DecodeBatch)
        m._h, m.n, m._keep, m.last_ms = h, n, None, ms.value
        return m

    def history_result(self, i):
        """(status, the request reduced to a frontier in the base document's LVs) of output i of a
        history batch."""
        return _frontier_result(lib().dtgpu_decode_history_result, self._h, i)

    def encode_from(self, docs, versions, opts=None):
        """ListOpLog::encode_from(opts, versions[i]) of document docs[i] for a whole batch, on the GPU
        (dtgpu_decode_encode_from): the `.dt` patch that takes a peer at versions[i] (any set of LVs;
        [] is ROOT) to this document's tip.  opts defaults to ENCODE_PATCH.  Returns a PatchBatch."""
        n = len(docs)
        if len(versions) != n:
            raise ValueError("one version per document index")
        d = (ctypes.c_uint32 * max(n, 1))(*[int(x) for x in docs])
        pv, po = _csr(versions, n)
        ms = ctypes.c_float()
        h = ctypes.c_void_p()
        flags = (opts or ENCODE_PATCH).flags()
        _check(lib().dtgpu_decode_encode_from(self._h, d, pv, po, n, flags, ctypes.byref(ms), ctypes.byref(h)))
        return PatchBatch(h, n, ms.value)

    def summarize_versions(self, i):
        """AgentAssignment::summarize_versions of resident document i (dtgpu_decode_summarize)."""
        return _read_summary(lambda *a: lib().dtgpu_decode_summarize(self._h, i, *a))

    def intersect(self, docs, summaries, frontiers=None, remote_frontier=False):
        """CausalGraph::intersect_with_summary for a whole batch, on the GPU (dtgpu_decode_intersect):
        summaries[i] (as ListOpLog.intersect_with_summary takes it; with remote_frontier a remote
        frontier [(name, seq)]) met with document docs[i]; frontiers[i] are extra LVs of that
        document.  Returns an IntersectBatch."""
        if len(summaries) != len(docs):
            raise ValueError("one summary per document index")
        sms = [summary_of_remote_frontier(x) if remote_frontier else normalize_summary(x) for x in summaries]
        S, names = _pack_summaries(sms, docs, frontiers)
        ms, h = ctypes.c_float(), ctypes.c_void_p()
        _check(lib().dtgpu_decode_intersect(self._h, ctypes.byref(S), len(docs), ctypes.byref(ms), ctypes.byref(h)))
        return IntersectBatch(h, len(docs), ms.value, names)

    def sync(self, docs, summaries, opts=None, frontiers=None):
        """The whole answer to a batch of sync hellos (dtgpu_decode_encode_from_summaries):
        (PatchBatch of what each peer lacks, IntersectBatch of the common frontiers and of what
        each peer has that this side lacks).  opts defaults to ENCODE_PATCH."""
        if len(summaries) != len(docs):
            raise ValueError("one summary per document index")
        S, names = _pack_summaries([normalize_summary(x) for x in summaries], docs, frontiers)
        ms, hp, hx = ctypes.c_float(), ctypes.c_void_p(), ctypes.c_void_p()
        flags = (opts or ENCODE_PATCH).flags()
        _check(lib().dtgpu_decode_encode_from_summaries(self._h, ctypes.byref(S), len(docs), flags, ctypes.byref(ms),
                                                        ctypes.byref(hp), ctypes.byref(hx)))
        return PatchBatch(hp, len(docs), ms.value), IntersectBatch(hx, len(docs), ms.value, names)

    def checkout_versions(self, docs, versions):
        """ListOpLog::checkout(versions[i]) of document docs[i] for a whole batch: the histories
        projected on the GPU (history), then one device-staged checkout batch.  Returns the
        ListBranch of every request (content, and the frontier in the base document's LVs); an
        output whose projection or checkout fails raises ParseError.  (ROOT requests are the empty
        branch: they are answered here, a zero-LV oplog is not staged.)"""
        live = [i for i, v in enumerate(versions) if len(v)]
        out = [ListBranch() for _ in versions]
        if not live:
            return out
        h = self.history([docs[i] for i in live], [versions[i] for i in live])
        fronts = []
        for k in range(len(live)):
            st, f = h.history_result(k)
            _check(st)
            fronts.append(f)
        b = h.checkout_batch()
        b.run()
        b.sync()
        for k, (i, r) in enumerate(zip(live, b.results())):
            _check(r["status"])
            out[i] = ListBranch(b.text(k), fronts[k])
        return out

    def xf_operations_from(self, docs, frm, merging):
        """ListOpLog::iter_xf_operations_from(frm[i], merging[i]) of document docs[i] for a whole
        batch, planned and replayed on the GPU (dtgpu_decode_xf_from): both are any sets of the
        document's LVs ([] is ROOT); documents may repeat.  Returns a MergeBatch."""
        n = len(docs)
        if len(frm) != n or len(merging) != n:
            raise ValueError("one from and one merging version per document index")
        pa, oa = _csr(frm, n)
        pb, ob = _csr(merging, n)
        d = (ctypes.c_uint32 * max(n, 1))(*[int(x) for x in docs])
        ms, h = ctypes.c_float(), ctypes.c_void_p()
        _check(lib().dtgpu_decode_xf_from(self._h, d, pa, oa, pb, ob, n, ctypes.byref(ms), ctypes.byref(h)))
        return MergeBatch(h, n, ms.value, self, [int(x) for x in docs])

    def merge(self, docs, branches, merging):
        """ListBranch::merge for a batch: branches[i] is a ListBranch of document docs[i], taken from
        its version to find_dominators_2(version, merging[i]).  A branch whose request failed is
        left as it was; ParseError for the first such request is raised after the others are
        updated."""
        m = self.xf_operations_from(docs, [b.version for b in branches], merging)
        bad = 0
        for i, b in enumerate(branches):
            st = m.status(i)
            if st:
                bad = bad or st
                continue
            b._content = m.content_bytes(i)
            b.version = m.version(i)
        _check(bad)
        return m

    def checkout_batch(self, blame=False, flags=0, seg_ops=0, seg_max=0, lds_fill=0):
        """A device-staged checkout Batch over these decoded (or merged) oplogs; consumes this
        handle (dtgpu_batch_create_decoded_opts).  blame, flags, seg_ops, seg_max, lds_fill: as
        Batch takes them."""
        h, self._h = self._h, None
        b = Batch.__new__(Batch)
        out = ctypes.c_void_p()
        opts = BatchOpts(0, 0, 0, int(flags) | (OPT_BLAME if blame else 0), int(seg_ops), int(seg_max), int(lds_fill))
        _check(lib().dtgpu_batch_create_decoded_opts(h, ctypes.byref(opts), ctypes.byref(out)))
        b._h, b.n, b._keep = out.value, self.n, None
        return b

    def blame_versions(self, docs, versions):
        """Blame at a version for a whole batch: who wrote each character of
        ListOpLog::checkout(versions[i]) of document docs[i].  As checkout_versions: the histories
        projected on the GPU (history), then one device-staged blame batch.  Returns (ListBranch,
        spans) per request, spans as Batch.blame_spans gives them; ROOT requests are (ListBranch(),
        []).  The projected oplog renumbers LVs, so the runs' LVs are not the base document's: the
        (agent_name, seq) spans are the answer that holds across numberings.  An output whose
        projection or checkout fails raises ParseError."""
        live = [i for i, v in enumerate(versions) if len(v)]
        out = [(ListBranch(), []) for _ in versions]
        if not live:
            return out
        h = self.history([docs[i] for i in live], [versions[i] for i in live])
        fronts = []
        for k in range(len(live)):
            st, f = h.history_result(k)
            _check(st)
            fronts.append(f)
        b = h.checkout_batch(blame=True)
        b.run()
        b.sync()
        for k, (i, r) in enumerate(zip(live, b.results())):
            _check(r["status"])
            out[i] = (ListBranch(b.text(k), fronts[k]), b.blame_spans(k))
        return out

    def profile(self, i):
        out = (ctypes.c_uint32 * 8)()
        _check(lib().dtgpu_decode_profile(self._h, i, out))
        return list(out)

    def bytes_in(self) -> int:
        return lib().dtgpu_decode_bytes(self._h, 0)

    def bytes_out(self) -> int:
        return lib().dtgpu_decode_bytes(self._h, 1)


class _ResultBatch:
    """What one per-request call over a DecodeBatch returned: a device-side handle of n requests,
    each with a status and a reduced frontier.  A subclass names its C functions (dtgpu_<_C>_result /
    _profile / _free) and the width of its profile record."""
    _C, _PROFILE = None, 8

    def __init__(self, handle, n, last_ms):
        self._h, self.n, self.last_ms = handle, n, last_ms

    def __len__(self):
        return self.n

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            getattr(lib(), f"dtgpu_{self._C}_free")(h)
            self._h = None

    def _result(self, i):
        return _frontier_result(getattr(lib(), f"dtgpu_{self._C}_result"), self._h, i)

    def status(self, i) -> int:
        return self._result(i)[0]

    def _profile(self, i):
        out = (ctypes.c_uint32 * self._PROFILE)()
        _check(getattr(lib(), f"dtgpu_{self._C}_profile")(self._h, i, out))
        return list(out)


class PatchBatch(_ResultBatch):
    """The patches of one DecodeBatch.encode_from call (dtgpu_patches), resident on the device."""
    _C, _PROFILE = "patches", 12

    def frontier(self, i):
        """Request i reduced to a frontier, in the base document's LVs, ascending."""
        return self._result(i)[1]

    def profile(self, i):
        """dtgpu_patches_profile: [mark form (1 LDS, 2 HBM), mark us, build us, walk steps, then --
        when DTGPU_PATCH_PROF was set at the call -- the build wave's cycles in its seven phases]."""
        return self._profile(i)

    def patch(self, i) -> bytes:
        """Request i's `.dt` patch; ParseError carries a non-zero status."""
        return _sized_bytes(lambda *a: lib().dtgpu_patches_get(self._h, i, *a))


class MergeBatch(_ResultBatch):
    """The merges of one DecodeBatch.xf_operations_from call (dtgpu_merges): per request the merged
    version, the transformed operations and the merged content."""
    _C = "merges"

    def __init__(self, handle, n, last_ms, base, docs):
        super().__init__(handle, n, last_ms)
        self._base, self._docs, self._arrays = base, docs, {}

    def version(self, i):
        """find_dominators_2(from, merging) in the base document's LVs, ascending."""
        st, f = self._result(i)
        _check(st)
        return f

    def xf_operations_lv(self, i):
        """[(lv, pos or None)] in application order: ListOpLog.xf_operations_lv(frm, merging)."""
        buf, n = _sized(lambda *a: lib().dtgpu_merges_ops(self._h, i, *a), lambda k: (ctypes.c_uint32 * max(2, 2 * k))())
        import numpy as np
        a = np.frombuffer(buf, dtype=np.uint32, count=2 * n).reshape(-1, 2).tolist()
        return [(lv, None if x == 0xFFFFFFFF else x) for lv, x in a]

    def iter_xf_operations(self, i):
        """What ListOpLog.iter_xf_operations(frm, merging) yields, from the resident document's
        arrays (DecodeBatch.export)."""
        d = self._docs[i]
        if d not in self._arrays:
            self._arrays[d] = (self._base.export(d, "ops"), bytes(self._base.export(d, "content")),
                               self._base.export(d, "char_offsets"))
        ops, content, coff = self._arrays[d]
        return merge_xf_runs(ops, content, coff, self.xf_operations_lv(i))

    def content_bytes(self, i) -> bytes:
        """The branch's content after the merge: the checkout at version(i)."""
        return _sized_bytes(lambda *a: lib().dtgpu_merges_text(self._h, i, *a))

    def profile(self, i):
        """dtgpu_merges_profile: the batch's us in mark + projection, prep, plan, replay, LV
        translation; then request i's commands, first reported command, reported LVs."""
        return self._profile(i)


class IntersectBatch(_ResultBatch):
    """The intersections of one DecodeBatch.intersect / sync call (dtgpu_intersect)."""
    _C = "intersect"

    def __init__(self, handle, n, last_ms, names):
        super().__init__(handle, n, last_ms)
        self._names = names

    def frontier(self, i):
        """The version request i's peer and the document share, in the document's LVs, ascending."""
        return self._result(i)[1]

    def remainder_records(self, i):
        """Request i's remainder as (entry index, start, end) records, in visiting order."""
        k = ctypes.c_size_t()
        lib().dtgpu_intersect_remainder(self._h, i, None, 0, ctypes.byref(k))
        buf = (ctypes.c_uint64 * max(1, 3 * k.value))()
        lib().dtgpu_intersect_remainder(self._h, i, buf, k.value, ctypes.byref(k))
        return [(buf[3 * j], buf[3 * j + 1], buf[3 * j + 2]) for j in range(k.value)]

    def remainder(self, i):
        """What request i's peer has and the document lacks: [(name, ranges)], or None."""
        return _group_remainder(self._names[i], self.remainder_records(i))

    def local_frontier(self, i):
        """frontier(i) of a remote-frontier request; KeyError when the document lacks part of it."""
        st, f = self._result(i)
        _check(st)
        rem = self.remainder(i)
        if rem is not None:
            raise KeyError(rem)
        return f

    def profile(self, i):
        """dtgpu_intersect_profile: [known pieces, remainder records, re-ordered ranges, count us,
        emit us, mark us, 0, 0]."""
        return self._profile(i)


GQ_KINDS = {"diff": 0, "conflict": 1, "contains": 2, "dominators": 3, "diff_level": 4, "conflict_level": 5}
DIFF_FLAGS = ["OnlyA", "OnlyB", "Shared"]


def graph_queries(graphs, queries, span_cap=512, timing=False, common_cap=None):
    """Batched causal-graph queries on the GPU (dtgpu_graph_queries, one wavefront per query).

    graphs: GraphEntrySimple lists ([{"span": [start, end], "parents": [...]}, ...]).
    queries: ("diff", g, a, b) -> (only_a, only_b) span lists, newest first (Graph::diff_rev);
             ("conflict", g, a, b) -> ([(start, end, flag)], common) (Graph::find_conflicting);
             ("contains", g, frontier, target) -> bool (frontier_contains_version; -1 = ROOT);
             ("dominators", g, a, b) -> sorted list (find_dominators_2 of two dominator sets);
             ("diff_level", g, a, b) -> as "diff", by level-synchronous propagation (dt_level.hip);
             ("conflict_level", g, a, b) -> as "conflict": level-synchronous marks + a bucketed sweep.
    Frontiers may be of any width.  A query the device could not answer yields ("error", status)."""
    hist, off = [], [0]
    for g in graphs:
        for e in g:
            hist += [e["span"][0], e["span"][1], len(e["parents"])] + list(e["parents"])
        off.append(len(hist))
    H = (ctypes.c_int64 * max(1, len(hist)))(*hist)
    O = (ctypes.c_size_t * len(off))(*off)
    nq = len(queries)
    Q = (GraphQuery * max(1, nq))()
    keep = []   # the frontier arrays the query structs point at
    for i, (kind, g, a, b) in enumerate(queries):
        q = Q[i]
        q.kind, q.graph, q.na = GQ_KINDS[kind], g, len(a)
        fa = (ctypes.c_int64 * max(1, len(a)))(*a)
        keep.append(fa)
        q.a = ctypes.cast(fa, ctypes.POINTER(ctypes.c_int64))
        if kind == "contains":
            q.target = b
        else:
            q.nb = len(b)
            fb = (ctypes.c_int64 * max(1, len(b)))(*b)
            keep.append(fb)
            q.b = ctypes.cast(fb, ctypes.POINTER(ctypes.c_int64))
    if common_cap is None:   # room for any answer: a common frontier / dominator set is never
        common_cap = max([2] + [len(a) + (0 if k == "contains" else len(b)) + 1 for k, _g, a, b in queries]
                         + [max([len(e["parents"]) for e in gr] or [0]) + 1 for gr in graphs])
    spans = (ctypes.c_int64 * (max(1, nq) * span_cap * 3))()
    common = (ctypes.c_int64 * (max(1, nq) * common_cap))()
    ans = (GraphAnswer * max(1, nq))()
    ms = ctypes.c_float()
    _check(lib().dtgpu_graph_queries(H, O, len(graphs), Q, nq, spans, span_cap, common, common_cap, ans,
                                     ctypes.byref(ms)))
    out = []
    for i, (kind, _g, _a, _b) in enumerate(queries):
        r = ans[i]
        if r.status:
            out.append(("error", r.status))
            continue
        base = 3 * span_cap * i
        tri = [(spans[base + 3 * k], spans[base + 3 * k + 1], spans[base + 3 * k + 2]) for k in range(r.n_a + r.n_b)]
        if kind in ("diff", "diff_level"):
            out.append(([(s, e) for s, e, _ in tri[:r.n_a]], [(s, e) for s, e, _ in tri[r.n_a:]]))
        elif kind in ("conflict", "conflict_level"):
            cb = common_cap * i
            out.append(([(s, e, DIFF_FLAGS[f]) for s, e, f in tri[:r.n_a]], list(common[cb:cb + r.n_common])))
        elif kind == "dominators":
            cb = common_cap * i
            out.append(list(common[cb:cb + r.n_common]))
        else:
            out.append(bool(r.n_a))
    return (out, ms.value) if timing else out


def batch_checkout(docs, **kw):
    """Checkout every `.dt` document in `docs`; returns (results, texts)."""
    b = Batch(docs=docs, **kw)
    b.run()
    b.sync()
    res = b.results()
    return res, [b.text(i) if r["status"] == 0 else None for i, r in enumerate(res)]


def batch_blame(docs, **kw):
    """Checkout every `.dt` document in `docs` with its blame; returns (results, texts, spans),
    spans[i] as Batch.blame_spans gives them (None for a document that failed)."""
    b = Batch(docs=docs, blame=True, **kw)
    b.run()
    b.sync()
    res = b.results()
    ok = [r["status"] == 0 for r in res]
    return (res, [b.text(i) if ok[i] else None for i in range(len(res))],
            [b.blame_spans(i) if ok[i] else None for i in range(len(res))])


def device_count() -> int:
    return lib().dtgpu_device_count()


def synth_ops(doc, target_ops=5000):
    """Op list of synthetic document `doc` (dt_synth.cpp): (n_agents, [(agent, kind, pos, len,
    text, parents)])."""
    na = ctypes.c_uint32()
    n = lib().dtgpu_synth_ops(doc, target_ops, ctypes.byref(na), None, 0)
    buf = (ctypes.c_uint32 * max(1, n))()
    lib().dtgpu_synth_ops(doc, target_ops, ctypes.byref(na), buf, n)
    w = list(buf[:n])
    ops, i = [], 0
    while i < n:
        agent, kind, pos, ln, c0, c1, np_ = w[i:i + 7]
        text = bytes([c0, c1][:ln]).decode() if kind == 0 else ""
        ops.append((agent, kind, pos, ln, text, w[i + 7:i + 7 + np_]))
        i += 7 + np_
    return na.value, ops


def synth_oplog(doc, target_ops=5000):
    """Synthetic document `doc` built as a ListOpLog."""
    h = ctypes.c_void_p()
    _check(lib().dtgpu_synth_oplog(doc, target_ops, ctypes.byref(h)))
    return ListOpLog(h.value)


def synth_merge_oplog(doc, target_ops=5000, n_agents=0):
    """SURVEY.md 8(d)4 synthetic document `doc` (dt_synth.cpp MergeGen: per-step pairwise merges
    with p = 0.1 via find_dominators_2, make_random_change edits), built as a ListOpLog.
    n_agents = 0 draws U{4..16}; a larger count gives a wide history (many causal chains)."""
    h = ctypes.c_void_p()
    _check(lib().dtgpu_synth_merge_oplog(doc, target_ops, n_agents, ctypes.byref(h)))
    return ListOpLog(h.value)


def apply_edits_push_merge(txns, agent_name="jeremy"):
    """crates/bench/src/utils.rs:25-44 (apply_edits_push_merge): a JSON trace's patches
    (pos, del, ins) pushed into a new ListOpLog by one agent at the current version, delete
    before insert.  The oplog the reference's benches and checkout_tip run on."""
    o = ListOpLog()
    a = o.get_or_create_agent_id(agent_name)
    for txn in txns:
        for pos, dl, ins in txn["patches"]:
            if dl:
                o.add_delete_without_content(a, pos, pos + dl)
            if ins:
                o.add_insert(a, pos, ins)
    return o
