"""The argument checks and the frontier readers of the per-request calls over a resident
DecodeBatch -- dtgpu_decode_history, dtgpu_decode_encode_from, dtgpu_decode_xf_from,
dtgpu_decode_intersect, dtgpu_decode_encode_from_summaries -- through raw ctypes calls on
dt_amd.lib(), entry for entry.

Every malformed request is DTGPU_ERR_ARG before anything is staged; whether `*out` is nulled on the
way differs per entry and is pinned as it is (NULLS_OUT).  One good call per entry then reads every
request's frontier through the entry's *_result function (width only, truncated, whole, index out
of range) and compares it with the host ListOpLog's dominators / intersect_with_summary."""
import ctypes

import pytest

import dt_amd

pytestmark = pytest.mark.gpu

ERR_ARG = 67
SENTINEL = 0xDEAD0
ENTRIES = ("history", "encode_from", "xf_from", "xf_merging", "intersect", "sync")
# dtgpu_decode_history leaves *out as it was when it rejects its arguments; the others null it first
NULLS_OUT = {"history": False, "encode_from": True, "xf_from": True, "xf_merging": True, "intersect": True, "sync": True}
RESULT = {"history": ("dtgpu_decode_size", "dtgpu_decode_history_result", "dtgpu_decode_free"),
          "patches": ("dtgpu_patches_size", "dtgpu_patches_result", "dtgpu_patches_free"),
          "merges": ("dtgpu_merges_size", "dtgpu_merges_result", "dtgpu_merges_free"),
          "intersect": ("dtgpu_intersect_size", "dtgpu_intersect_result", "dtgpu_intersect_free")}
HANDLES = {"history": ("history",), "encode_from": ("patches",), "xf_from": ("merges",), "xf_merging": ("merges",),
           "intersect": ("intersect",), "sync": ("patches", "intersect")}


def _doc(first, second):
    o = dt_amd.ListOpLog()
    a, b = o.get_or_create_agent_id("a"), o.get_or_create_agent_id("b")
    o.add_insert_at(a, [], 0, first)
    o.add_insert_at(b, [], 0, second)
    return o.encode()


@pytest.fixture(scope="module")
def resident():
    """(host oplogs, decoded batch, a batch that was never run) of two documents of a dozen LVs,
    each with a tip two LVs wide."""
    files = [_doc("aaaaaaaa", "bbbb"), _doc("hello world", "xy")]
    hosts = [dt_amd.ListOpLog.load_from(f) for f in files]
    base = dt_amd.DecodeBatch(files)
    base.run()
    assert all(base.status(i)["status"] == 0 and len(hosts[i].local_frontier()) == 2 for i in (0, 1))
    return hosts, base, dt_amd.DecodeBatch(files)


def _arr(t, xs):
    return (t * max(1, len(xs)))(*xs)


def _call(entry, base, docs, off, vals, null_out=()):
    """One raw call of `entry` with the request (docs, CSR off / vals); docs None: n = 0 and null
    arrays; vals None: a null value pointer.  Returns (status, the out handles' values after)."""
    L = dt_amd.lib()
    n = 0 if docs is None else len(docs)
    pd = None if docs is None else _arr(ctypes.c_uint32, docs)
    po = None if off is None else _arr(ctypes.c_size_t, off)
    pv = None if vals is None else _arr(ctypes.c_uint64, vals)
    zero = None if docs is None else _arr(ctypes.c_size_t, [0] * (n + 1))
    ms = ctypes.c_float()
    outs = [ctypes.c_void_p(SENTINEL) for _ in HANDLES[entry]]
    refs = [None if k in null_out else ctypes.byref(o) for k, o in enumerate(outs)]
    if entry == "history":
        st = L.dtgpu_decode_history(base._h, pd, pv, po, n, ctypes.byref(ms), refs[0])
    elif entry == "encode_from":
        st = L.dtgpu_decode_encode_from(base._h, pd, pv, po, n, dt_amd.ENCODE_PATCH.flags(), ctypes.byref(ms), refs[0])
    elif entry == "xf_from":
        st = L.dtgpu_decode_xf_from(base._h, pd, pv, po, _arr(ctypes.c_uint64, []), zero, n, ctypes.byref(ms), refs[0])
    elif entry == "xf_merging":
        st = L.dtgpu_decode_xf_from(base._h, pd, _arr(ctypes.c_uint64, []), zero, pv, po, n, ctypes.byref(ms), refs[0])
    else:
        S = None
        if docs is not None:
            S, _ = dt_amd._pack_summaries([[] for _ in docs], [0] * n)
            S.doc = pd
            S.version_off = po
            S.versions = pv
            S = ctypes.byref(S)
        if entry == "intersect":
            st = L.dtgpu_decode_intersect(base._h, S, n, ctypes.byref(ms), refs[0])
        else:
            st = L.dtgpu_decode_encode_from_summaries(base._h, S, n, dt_amd.ENCODE_PATCH.flags(), ctypes.byref(ms),
                                                      refs[0], refs[1])
    return st, [o.value for o in outs]


def _free(entry, handles):
    for kind, h in zip(HANDLES[entry], handles):
        getattr(dt_amd.lib(), RESULT[kind][2])(ctypes.c_void_p(h))


@pytest.mark.parametrize("entry", ENTRIES)
def test_rejected_requests(resident, entry):
    hosts, base, unrun = resident
    after = None if NULLS_OUT[entry] else SENTINEL
    bad = {"doc == n": ([0, 2], [0, 1, 2], [3, 3]),
           "descending offsets": ([0, 1], [0, 2, 1], [3, 3]),
           "descending first pair": ([0, 1], [1, 0, 1], [3, 3]),
           "null values": ([0, 1], [0, 1, 2], None)}
    for name, (docs, off, vals) in bad.items():
        st, outs = _call(entry, base, docs, off, vals)
        assert st == ERR_ARG and outs == [after] * len(outs), (name, st, outs)
    st, outs = _call(entry, unrun, [0, 1], [0, 1, 2], [3, 3])
    assert st == ERR_ARG and outs == [after] * len(outs), ("not run", st, outs)
    for k in range(len(HANDLES[entry])):
        st, outs = _call(entry, base, [0, 1], [0, 1, 2], [3, 3], null_out=(k,))
        # the handle that was passed is nulled (or left) as for any other rejected request
        assert st == ERR_ARG and outs == [SENTINEL if j == k else after for j in range(len(outs))], (k, st, outs)
    if entry in ("intersect", "sync"):   # the summaries' own CSR
        S, _ = dt_amd._pack_summaries([[], []], [0, 1])
        S.entry_off = _arr(ctypes.c_size_t, [0, 1, 0])
        L, ms = dt_amd.lib(), ctypes.c_float()
        outs = [ctypes.c_void_p(SENTINEL), ctypes.c_void_p(SENTINEL)]
        if entry == "intersect":
            st = L.dtgpu_decode_intersect(base._h, ctypes.byref(S), 2, ctypes.byref(ms), ctypes.byref(outs[0]))
        else:
            st = L.dtgpu_decode_encode_from_summaries(base._h, ctypes.byref(S), 2, 0, ctypes.byref(ms),
                                                      ctypes.byref(outs[0]), ctypes.byref(outs[1]))
        assert st == ERR_ARG and outs[0].value is None


@pytest.mark.parametrize("entry", ENTRIES)
def test_empty_batch(resident, entry):
    hosts, base, unrun = resident
    st, outs = _call(entry, base, None, None, None)
    assert st == 0 and all(outs) and SENTINEL not in outs, (st, outs)
    for kind, h in zip(HANDLES[entry], outs):
        size, result, _ = RESULT[kind]
        L = dt_amd.lib()
        assert getattr(L, size)(ctypes.c_void_p(h)) == 0
        assert getattr(L, result)(ctypes.c_void_p(h), 0, None, 0, None) == ERR_ARG
    _free(entry, outs)


@pytest.mark.parametrize("entry", ENTRIES)
def test_frontier_readers(resident, entry):
    hosts, base, unrun = resident
    tips = [h.local_frontier() for h in hosts]
    docs = [0, 1, 0, 1]
    sets = [tips[0], [3], [], [tips[1][1], 2, tips[1][0], 2]]
    off = [5]   # the CSR need not start at 0 where the parent allows it (history, encode_from, xf_from)
    if entry in ("intersect", "sync"):
        off = [0]
    assert [len(hosts[d].dominators(s)) for d, s in zip(docs, sets)] == [2, 1, 0, 2]
    vals = [0] * off[0]
    for s in sets:
        vals += s
        off.append(len(vals))
    st, outs = _call(entry, base, docs, off, vals)
    assert st == 0 and all(outs), (st, outs)
    L = dt_amd.lib()
    for kind, h in zip(HANDLES[entry], outs):
        size, result, _ = RESULT[kind]
        h = ctypes.c_void_p(h)
        read = getattr(L, result)
        assert getattr(L, size)(h) == len(docs)
        for i, (d, s) in enumerate(zip(docs, sets)):
            if kind == "intersect":
                want = hosts[d].intersect_with_summary([], s)[0]
            else:
                want = hosts[d].dominators(s)
            k = ctypes.c_size_t(99)
            assert read(h, i, None, 0, ctypes.byref(k)) == 0 and k.value == len(want), (kind, i)   # the width only
            buf = (ctypes.c_uint64 * 4)(*[SENTINEL] * 4)
            k = ctypes.c_size_t(99)
            assert read(h, i, buf, 4, ctypes.byref(k)) == 0 and list(buf[:k.value]) == want, (kind, i, list(buf), want)
            assert list(buf[k.value:]) == [SENTINEL] * (4 - k.value)
            assert read(h, i, buf, 4, None) == 0
            if len(want) == 2:   # a cap below the width truncates and still reports the width
                buf = (ctypes.c_uint64 * 2)(SENTINEL, SENTINEL)
                k = ctypes.c_size_t(99)
                assert read(h, i, buf, 1, ctypes.byref(k)) == 0 and k.value == 2 and list(buf) == [want[0], SENTINEL]
            assert read(h, i, None, 1, None) == ERR_ARG
        k = ctypes.c_size_t(99)
        assert read(h, len(docs), None, 0, ctypes.byref(k)) == ERR_ARG
        assert k.value == (99 if kind == "history" else 0)   # the history reader leaves *n_frontier on a bad index
    _free(entry, outs)


def test_result_readers_reject_the_other_kind_of_handle(resident):
    """dtgpu_decode_history_result takes history handles only, dtgpu_decode_add_result handles that
    dtgpu_decode_add made only.  (Before the readers shared one FrontierSet, add_result on a history
    handle read a frontier arena that was never allocated; it is DTGPU_ERR_ARG now, as
    history_result on a merged handle always was.)"""
    hosts, base, unrun = resident
    L = dt_amd.lib()
    h = base.history([0], [[3]])
    m = base.add([o.encode_from(o.local_frontier(), dt_amd.ENCODE_PATCH) for o in hosts])   # nothing new
    k = ctypes.c_size_t(99)
    assert L.dtgpu_decode_add_result(h._h, 0, None, 0, ctypes.byref(k)) == ERR_ARG and k.value == 99
    assert L.dtgpu_decode_history_result(m._h, 0, None, 0, ctypes.byref(k)) == ERR_ARG and k.value == 99
    assert L.dtgpu_decode_history_result(base._h, 0, None, 0, ctypes.byref(k)) == ERR_ARG and k.value == 99
    assert L.dtgpu_decode_add_result(base._h, 0, None, 0, ctypes.byref(k)) == ERR_ARG and k.value == 99
    assert h.history_result(0) == (0, [3])
    assert L.dtgpu_decode_add_result(m._h, 2, None, 0, ctypes.byref(k)) == ERR_ARG and k.value == 99
