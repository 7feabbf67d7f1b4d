"""Batched blame (dt_blame.hip, Batch(blame=True)): who wrote each character, as maximal runs
(lv, len, agent, seq) in text order.  Every expected value is the CPU oracle's (tests/blame_docs.py:
the oracle's transformed operations applied to a list of LVs, mapped through its agent runs and
grouped); tests/test_blame_docs.py pins that model on the CPU.  The same runs must come out of
every replay path -- the flat and 3-level LDS tiers, the HBM tier, the LDS -> HBM hand-back, cut
replay, the fast-forward path -- through host and device staging, decoded handles and reruns, and
the text, length and hash of a blame batch must be those of a plain batch."""
import ctypes
import random

import pytest

import blame_docs as BD
import golden_data as G
import linear_docs
import merge_docs
from oracle.oracle import OpLog as OracleOpLog

pytestmark = pytest.mark.gpu

import dt_amd  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if dt_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the engine has no CPU fallback")


_MODEL = {}


def model(data):
    """(runs, text) of a document's blame at the tip by the CPU model, computed once per document."""
    if data not in _MODEL:
        ora = OracleOpLog.load_from(data)
        _MODEL[data] = (BD.model_runs(ora), ora.checkout_tip_bytes())
    return _MODEL[data]


def run_both(docs, staging="host", timed=0, **kw):
    """The blame batch and a plain batch of the same documents, both run: (blame batch, plain)."""
    out = []
    for blame in (True, False):
        b = dt_amd.Batch(docs=docs, staging=staging, blame=blame, **kw)
        if timed:
            for _ in range(timed):
                b.run_timed()
        else:
            b.run()
            b.sync()
        out.append(b)
    return out


def check_doc(b, i, data):
    """Document i of blame batch b against the model of `data`: runs, names, spans, text."""
    runs, text = model(data)
    names = b.blame_agents(i)
    got = b.blame(i)
    assert [(lv, n, names[a].decode(), seq) for lv, n, a, seq in got] == runs
    spans = b.blame_spans(i)
    assert spans == BD.spans_of(runs)
    assert b.text(i) == text
    assert sum(n for _lv, n, _a, _s in got) == len(text.decode())
    return got


def check_all(docs, staging="host", timed=0, **kw):
    b, plain = run_both(docs, staging, timed, **kw)
    res = b.results()
    assert res == plain.results()   # the unchanged product: status, length, hash, LVs
    for i, d in enumerate(docs):
        assert res[i]["status"] == 0, (i, res[i])
        assert b.text(i) == plain.text(i)
        check_doc(b, i, d)
    return b


SMALL = BD.small_docs()


@pytest.mark.parametrize("flags", [0, dt_amd.OPT_NO_FAST_FORWARD], ids=["ff", "tracker"])
@pytest.mark.parametrize("staging", ["host", "device"])
def test_run_arithmetic_at_the_scan_widths(staging, flags):
    """One-author texts of 1 .. 1,025 characters typed as one run (one output run) and by two agents
    alternating character by character through the graph (as many runs as characters: head flags,
    scan carries and the emit cross every wave and workgroup-round boundary).  Both forms are
    linear histories: on the fast-forward path one piece holds every agent run, and with that
    path off the tracker's list has a head at every entry."""
    docs = [SMALL[f"{kind}_{n}"] for kind in ("one_run", "alternating") for n in BD.WIDTHS]
    b = check_all(docs, staging, flags=flags)
    k = len(BD.WIDTHS)
    assert [len(b.blame(i)) for i in range(k)] == [1] * k
    assert [len(b.blame(k + i)) for i in range(k)] == BD.WIDTHS
    assert b.fast_forwarded() == [0 if flags else 1] * (2 * k)


@pytest.mark.parametrize("flags", [0, dt_amd.OPT_NO_FAST_FORWARD], ids=["ff", "tracker"])
@pytest.mark.parametrize("staging", ["host", "device"])
def test_small_documents(staging, flags):
    """Splitting and joining, agent boundaries inside consecutive LVs, the tie-break KAT, UTF-8, the
    linear turns: the one-agent documents on the fast-forward path and, with it off, on the tracker."""
    names = sorted(SMALL)
    b = check_all([SMALL[k] for k in names], staging, flags=flags)
    n = {k: len(b.blame(i)) for i, k in enumerate(names)}
    assert n["deleted_middle"] == 2 and n["insert_in_middle"] == 3 and n["insert_deleted_again"] == 1
    assert n["all_deleted"] == 0 and n["all_deleted_concurrently"] == 0 and n["no_inserts"] == 0
    assert n["agent_boundary"] == 2 and n["tie_break"] == 3
    assert b.blame(names.index("insert_deleted_again")) == [(0, 5, 0, 0)]
    ff = dict(zip(names, b.fast_forwarded()))
    assert ff["linear_turns"] == ff["linear_long"] == ff["deleted_middle"] == (0 if flags else 1)
    st = b.blame_stats()
    assert st["runs"] == sum(n.values()) and st["chars"] == sum(len(b.text(i).decode()) for i in range(len(names)))
    assert st["arena_bytes"] >= 16 * st["runs"]


@pytest.mark.parametrize("staging", ["host", "device"])
def test_batch_of_empty_texts(staging):
    """No document of the batch has a run: the run arena is empty, the reads are not."""
    docs = [SMALL["all_deleted"], SMALL["all_deleted_concurrently"], SMALL["no_inserts"]]
    b = check_all(docs, staging)
    assert [b.blame(i) for i in range(3)] == [[], [], []]
    st = b.blame_stats()
    assert st["runs"] == 0 and st["chars"] == 0


def test_utf8_spans_index_characters():
    b = check_all([SMALL["utf8"]])
    text = b.text(0).decode()
    spans = b.blame_spans(0)
    assert spans[-1][4] == len(text) < len(b.text(0))
    assert [text[s[3]:s[4]] for s in spans] and "".join(text[s[3]:s[4]] for s in spans) == text
    assert all(s[2] - s[1] == s[4] - s[3] for s in spans)


@pytest.mark.parametrize("staging", ["host", "device"])
def test_friendsforever_flat_tier(staging):
    data = G.dt_bytes("friendsforever")
    b = check_all([data, SMALL["tie_break"], data], staging, flags=dt_amd.OPT_NO_SEGMENTS)
    assert b.doc_stats(0)["lds_index"] == 1 and b.segments(0) == []
    assert b.blame(0) == b.blame(2)


@pytest.mark.parametrize("staging", ["host", "device"])
def test_three_level_lds_tier(staging):
    """60,000 inserted characters: the index estimate is past the flat tier's."""
    b = check_all([BD.two_blocks(30000), SMALL["tie_break"]], staging)
    assert b.doc_stats(0)["lds_index"] == 1
    assert [r[1] for r in b.blame(0)] == [30000, 30000]


def test_three_level_index_on_friendsforever(monkeypatch):
    monkeypatch.setenv("DTGPU_FLAT", "0")
    b = check_all([G.dt_bytes("friendsforever")], "device", flags=dt_amd.OPT_NO_SEGMENTS)
    assert b.doc_stats(0)["lds_index"] == 1 and b.segments(0) == []


@pytest.mark.parametrize("staging", ["host", "device"])
def test_hbm_tier(staging):
    """800,000 inserted characters: no LDS tier holds the index estimate."""
    b = check_all([BD.two_blocks(400000), SMALL["agent_boundary"]], staging)
    assert b.doc_stats(0)["lds_index"] == 0
    assert [r[1] for r in b.blame(0)] == [400000, 400000]


@pytest.mark.parametrize("staging", ["host", "device"])
def test_lds_handback(monkeypatch, staging):
    """An LDS index sized far too small: the documents overflow it and replay again from scratch on
    the HBM tier, which must still end with a correct list."""
    monkeypatch.setenv("DTGPU_LDS_FILL", "4000")
    data = G.dt_bytes("friendsforever")
    b = check_all([data, SMALL["tie_break"], data], staging, flags=dt_amd.OPT_NO_SEGMENTS)
    assert b.doc_stats(0)["lds_index"] == 0 and b.segments(0) == []


def _segments_holding(b, i, data):
    """The segments of document i whose LV ranges hold characters of the final text."""
    segs = b.segments(i)
    held = set()
    for lv, _n, _a, _s in model(data)[0]:
        held.add(next(k for k, s in enumerate(segs) if s["lo"] <= lv < s["hi"]))
    return segs, held


@pytest.mark.parametrize("staging", ["host", "device"])
def test_forced_cut_replay(monkeypatch, staging):
    """friendsforever cut into at least four segments: the final list is the last segment's, its
    placeholders resolved across at least three of them."""
    monkeypatch.setenv("DTGPU_SEG_OPS", "300")
    data = G.dt_bytes("friendsforever")
    b = check_all([data, data], staging)
    segs, held = _segments_holding(b, 0, data)
    assert len(segs) >= 4 and all(s["status"] == 0 for s in segs)
    assert len(held) >= 3


def test_cut_replay_handback(monkeypatch):
    monkeypatch.setenv("DTGPU_SEG_OPS", "300")
    monkeypatch.setenv("DTGPU_LDS_FILL", "4000")
    data = G.dt_bytes("friendsforever")
    b = check_all([data], "device")
    assert len(b.segments(0)) >= 4


@pytest.mark.parametrize("cut", [False, True], ids=["whole", "cut"])
def test_run_timed_twice(monkeypatch, cut):
    """A rerun replays, combines and counts again from scratch: the same runs."""
    if cut:
        monkeypatch.setenv("DTGPU_SEG_OPS", "300")
    data = G.dt_bytes("friendsforever")
    docs = [data, SMALL["linear_turns"], SMALL["tie_break"]]
    b = dt_amd.Batch(docs=docs, staging="device", blame=True, flags=0 if cut else dt_amd.OPT_NO_SEGMENTS)
    b.run_timed()
    first = [b.blame(i) for i in range(3)]
    b.run_timed()
    assert [b.blame(i) for i in range(3)] == first
    for i, d in enumerate(docs):
        check_doc(b, i, d)
    assert bool(b.segments(0)) == cut
    e2e = b.run_e2e_timed()
    assert len(e2e) == 4 and [b.blame(i) for i in range(3)] == first


@pytest.mark.parametrize("staging", ["host", "device"])
def test_linear_documents(staging):
    """The fast-forward path: pieces split at agent-run boundaries (one piece spans more than two
    agent runs), adjacent pieces of consecutive LVs joined, several segments composed."""
    docs = [linear_docs.random_linear(3, 150)[0], linear_docs.random_linear(4, 400, unicode=False)[0],
            linear_docs.sized_linear(130)[0], linear_docs.sized_linear(64, 1)[0],
            SMALL["linear_turns"], SMALL["linear_long"]]
    b = check_all(docs, staging)
    assert b.fast_forwarded() == [1] * len(docs)
    first = b.blame_spans(4)[:3]
    assert [s[0] for s in first] == [b"ann", b"bob", b"ann"] and first[2][3] == 3


@pytest.mark.parametrize("staging", ["host", "device"])
def test_mixed_batch(monkeypatch, staging):
    """Linear, plain and cut documents together: each has the blame of its own one-document batch
    (which the model is)."""
    monkeypatch.setenv("DTGPU_SEG_OPS", "300")
    data = G.dt_bytes("friendsforever")
    docs = [SMALL["linear_long"], data, SMALL["tie_break"], SMALL["utf8"], linear_docs.random_linear(5, 100)[0],
            SMALL["alternating_257"], data, SMALL["all_deleted"]]
    b = check_all(docs, staging)
    assert len(b.segments(1)) >= 4 and b.segments(2) == []
    ff = b.fast_forwarded()
    assert ff[0] == 1 and ff[1] == 0 and ff[4] == 1


def _check_versions(data, versions):
    ora = OracleOpLog.load_from(data)
    d = dt_amd.DecodeBatch([data])
    d.run()
    got = d.blame_versions([0] * len(versions), versions)
    assert len(got) == len(versions)
    for v, (branch, spans) in zip(versions, got):
        assert spans == BD.spans_of(BD.model_runs(ora, v)), v
        assert branch.content_bytes() == ora.checkout_bytes(list(v)), v
        if not v:
            assert (branch.content_bytes(), spans) == (b"", [])


def test_blame_at_every_version_of_the_small_document():
    data = merge_docs.small_bytes()
    vs = merge_docs.versions(dt_amd.ListOpLog.load_from(data))
    assert len(vs) == 38
    _check_versions(data, vs)


def test_blame_at_versions_of_friendsforever():
    data = G.dt_bytes("friendsforever")
    o = dt_amd.ListOpLog.load_from(data)
    rng = random.Random(11)
    vs = [[], o.local_frontier()] + [[rng.randrange(len(o))] for _ in range(6)]
    _check_versions(data, vs)


def test_one_document_forms():
    data = merge_docs.small_bytes()
    ora = OracleOpLog.load_from(data)
    o = dt_amd.ListOpLog.load_from(data)
    assert o.blame() == BD.spans_of(BD.model_runs(ora))
    assert o.blame([7]) == BD.spans_of(BD.model_runs(ora, [7])) and o.blame([]) == []
    res, texts, spans = dt_amd.batch_blame([data, b"not a dt file"])
    assert [r["status"] for r in res] == [0, 1] and texts[1] is None and spans[1] is None
    assert spans[0] == BD.spans_of(BD.model_runs(ora))


def test_after_decode_add():
    """checkout_batch(blame=True) on a merged handle: a history delivered as a prefix and a patch
    has the authorship of the whole document.  (The merge may number LVs differently: compared by
    (agent name, seq).)"""
    pairs = []
    for data, v in ((merge_docs.small_bytes(), [7]), (G.dt_bytes("friendsforever"), [9000]), (SMALL["linear_turns"], [80])):
        full = dt_amd.ListOpLog.load_from(data)
        pairs.append((data, full.history(v).encode(), full.encode_from(v, dt_amd.ENCODE_PATCH)))
    d = dt_amd.DecodeBatch([base for _, base, _ in pairs])
    d.run()
    m = d.add([patch for _, _, patch in pairs])
    assert all(m.add_result(i)[0] == 0 for i in range(len(pairs)))
    b = m.checkout_batch(blame=True)
    b.run()
    b.sync()
    for i, (data, _, _) in enumerate(pairs):
        runs, text = model(data)
        assert b.results()[i]["status"] == 0
        assert b.text(i) == text
        assert b.blame_spans(i) == BD.spans_of(runs), i


def _raw_blame(b, i):
    n = ctypes.c_size_t(99)
    st = dt_amd.lib().dtgpu_batch_blame(b._h, i, None, 0, ctypes.byref(n))
    return st, n.value


@pytest.mark.parametrize("staging", ["host", "device"])
def test_errors(staging):
    good = SMALL["tie_break"]
    bad = bytearray(G.COMPAT_SIMPLE_1)
    bad[-1] ^= 0xFF
    docs = [good, b"not a dt file", G.dt_bytes("friendsforever"), bytes(bad), SMALL["linear_turns"]]
    b, plain = run_both(docs, staging)
    res = b.results()
    assert res == plain.results() and [r["status"] for r in res] == [0, 1, 0, 18, 0]
    for i in (1, 3):   # a corrupt document: its own status, zero runs
        assert _raw_blame(b, i) == (res[i]["status"], 0)
        with pytest.raises(dt_amd.ParseError) as e:
            b.blame(i)
        assert e.value.code == res[i]["status"]
    for i in (0, 2, 4):
        check_doc(b, i, docs[i])
    # a plain batch has no blame; out of range; not with transformed-ops batches
    for call in (lambda: plain.blame(0), lambda: plain.blame_agents(0), lambda: plain.blame_stats(),
                 lambda: b.blame(len(docs))):
        with pytest.raises(dt_amd.ParseError) as e:
            call()
        assert e.value.code == 67 and e.value.name == "ErrArg"
    with pytest.raises(dt_amd.ParseError) as e:
        dt_amd.Batch(oplogs=[dt_amd.ListOpLog.load_from(good)], xf=True, blame=True)
    assert e.value.name == "ErrArg"
