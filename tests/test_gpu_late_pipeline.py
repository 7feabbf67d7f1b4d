"""The late pipeline: a device-staged batch whose smallest LDS tier holds more
than one resident round of documents prepares, plans and replays the documents past the first
round on side streams, so that the first round's replay does not wait for them.  DTGPU_LATE_FROM shrinks the
resident round so that a 40-document batch takes the path a real device reaches past ~8k documents.
Every text must equal the golden / oracle text: with the pipeline forced, off, with late
documents that cannot be cut, with the LDS -> HBM hand-back from the late launch, through the
timed entry points, and with a split pass taking precedence."""
import pytest

import golden_data as G
from synth_docs import phased_doc
from oracle.oracle import OpLog as OracleOpLog

pytestmark = pytest.mark.gpu

import dt_amd  # noqa: E402

N, FROM = 40, 32
LATE = list(range(FROM, N))   # equal documents keep their order: the last eight are late


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if dt_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the engine has no CPU fallback")


@pytest.fixture(scope="module")
def ff_want():
    w = G.trace("friendsforever_flat")["endContent"].encode()
    return w, (len(w), dt_amd.text_hash(w))


def _ff_batch(monkeypatch, pipe=True, **env):
    monkeypatch.setenv("DTGPU_LATE_FROM", str(FROM))
    # (a batch this small would cut every friendsforever copy by the fair-share rule, as a 10k
    # batch does not: only the late documents' single cut is left on)
    monkeypatch.setenv("DTGPU_SEG_OPS", "1000000")
    if not pipe:
        monkeypatch.setenv("DTGPU_LATE_PIPE", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return dt_amd.Batch(docs=[G.dt_bytes("friendsforever")] * N, staging="device")


def _assert_golden(b, key):
    res = b.results()
    assert [r["status"] for r in res] == [0] * len(res), [(i, r) for i, r in enumerate(res) if r["status"]]
    assert all((r["text_len"], r["text_hash"]) == key for r in res)


def test_forced_late_set_matches_golden(monkeypatch, ff_want):
    want, key = ff_want
    b = _ff_batch(monkeypatch)
    assert b.late_pipelined() == [0] * FROM + [1] * (N - FROM)
    for _ in range(3):   # every pass plans the late cuts again (a pass without them: ErrCheckout site 30)
        b.run()
        b.sync()
        _assert_golden(b, key)
    assert [i for i in range(N) if b.segments(i)] == LATE
    for i in LATE:
        segs = b.segments(i)
        assert len(segs) == 2 and all(s["status"] == 0 and s["host_fallback"] == 0 for s in segs), segs
    assert b.text(0) == want and b.text(N - 1) == want


def test_first_round_documents_cut_too(monkeypatch, ff_want):
    """At the default segment size a small batch cuts every copy: the main pipeline plans the
    first round's cut groups, the late pipeline its own."""
    want, key = ff_want
    monkeypatch.setenv("DTGPU_LATE_FROM", str(FROM))
    b = dt_amd.Batch(docs=[G.dt_bytes("friendsforever")] * N, staging="device")
    assert sum(b.late_pipelined()) == N - FROM
    for _ in range(2):
        b.run()
        b.sync()
        _assert_golden(b, key)
    assert all(len(b.segments(i)) >= 2 for i in range(N))
    assert b.text(1) == want and b.text(N - 2) == want


def test_pipeline_off_equals_on(monkeypatch, ff_want):
    want, key = ff_want
    on = _ff_batch(monkeypatch)
    on.run()
    on.sync()
    off = _ff_batch(monkeypatch, pipe=False)
    assert off.late_pipelined() == [0] * N
    off.run()
    off.sync()
    assert off.results() == on.results()
    _assert_golden(off, key)
    for i in range(N):
        assert off.text(i) == on.text(i) == want, i
    assert [i for i in range(N) if off.segments(i)] == LATE   # (cut either way: only the pipeline differs)
    for i in (0, LATE[0]):
        assert off.plan(i) == on.plan(i), i
        assert len(on.plan(i)[0]) > 0


def test_late_documents_that_cannot_be_cut(monkeypatch):
    """The four shortest documents have fewer than 128 op runs: late, but replayed whole."""
    monkeypatch.setenv("DTGPU_LATE_FROM", str(FROM))
    docs = [phased_doc(s) for s in range(36)]
    tiny = [phased_doc(100 + s, phases=1) for s in range(4)]
    docs[5:5] = tiny[:2]
    docs += tiny[2:]
    where = [5, 6, 38, 39]
    b = dt_amd.Batch(docs=docs, staging="device")
    late = b.late_pipelined()
    assert sum(late) == N - FROM and all(late[i] for i in where), late
    b.run()
    b.sync()
    res = b.results()
    for i, d in enumerate(docs):
        assert res[i]["status"] == 0, (i, res[i])
        assert b.text(i) == OracleOpLog.load_from(d).checkout_tip_bytes(), i
    assert all(b.segments(i) == [] for i in where)


def test_lds_handback_from_the_late_launch(monkeypatch, ff_want):
    """An LDS index sized far too small: both launches hand documents back, and the HBM tier
    replays them after the join."""
    want, key = ff_want
    b = _ff_batch(monkeypatch, DTGPU_LDS_FILL="4000")
    assert sum(b.late_pipelined()) == N - FROM
    b.run()
    b.sync()
    _assert_golden(b, key)
    assert all(b.text(i) == want for i in LATE)
    assert any(s["lds_index"] == 0 for i in LATE for s in b.segments(i))   # replayed on the HBM index


def test_timed_and_e2e_entry_points(monkeypatch, ff_want):
    want, key = ff_want
    b = _ff_batch(monkeypatch)
    ms = b.run_timed()
    _assert_golden(b, key)
    times = b.last_times()
    print("run_timed", ms, "last_times (plan, replay, prep)", times)
    assert all(t > 0 for t in times)
    assert sum(times) <= ms * (1 + 1e-5)   # (replay is the pass less prep and plan, in float32)
    e2e = b.run_e2e_timed()
    print("run_e2e_timed (decode, prep, plan, replay)", e2e)
    assert len(e2e) == 4 and all(t > 0 for t in e2e)
    _assert_golden(b, key)
    assert b.text(LATE[-1]) == want


def test_split_pass_takes_precedence(monkeypatch, ff_want):
    """A big-tier document beside flat-tier ones: a split pass, and no late pipeline with it."""
    want, key = ff_want
    monkeypatch.setenv("DTGPU_LATE_FROM", "2")
    big = G.dt_bytes("node_nodecc")
    docs = [big] + [G.dt_bytes("friendsforever")] * 5
    b = dt_amd.Batch(docs=docs, staging="device")
    assert b.late_pipelined() == [0] * len(docs)
    b.run()
    b.sync()
    res = b.results()
    assert [r["status"] for r in res] == [0] * len(docs), res
    assert b.text(0) == OracleOpLog.load_from(big).checkout_tip_bytes()
    assert all((r["text_len"], r["text_hash"]) == key for r in res[1:])
    assert b.text(len(docs) - 1) == want
