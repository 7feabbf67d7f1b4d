"""The replay's lane flags on the device (dt_replay.hip F_LIVE / F_VIS: a block held in registers
carries each item's liveness and visibility in the two top bits of its lane's word).  The documents
of tests/lane_flag_docs.py -- tests/test_lane_flag_docs.py asserts the corners they reach -- are
checked out in one batch and every text compared with the oracle's: by the release kernel and by
the instrumented one (DTGPU_DEBUG=1, which after every command compares the cached block's flags
with flags recomputed from the counts, code 214), replayed whole and as forced segments (so that
placeholder ids pass through the flag bits), staged by the device and by the host, and on the HBM
tier.  DTGPU_DEBUG=2 counts the paths the documents are built for."""
import pytest

import lane_flag_docs as D
from oracle.oracle import OpLog as OracleOpLog

pytestmark = pytest.mark.gpu

import dt_amd  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if dt_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the engine has no CPU fallback")


@pytest.fixture(scope="module")
def docs():
    """(names, .dt bytes, oracle texts)"""
    oplogs = D.all_docs()
    data = [o.encode() for o in oplogs.values()]
    return list(oplogs), data, [OracleOpLog.load_from(d).checkout_tip_bytes() for d in data]


def _run(b, n):
    b.run()
    b.sync()
    res = b.results()
    assert [r["status"] for r in res] == [0] * n, [(i, r, b.doc_stats(i)) for i, r in enumerate(res) if r["status"]]
    return [b.text(i) for i in range(n)]


def _tiers(b, i):
    return {s["lds_index"] for s in b.segments(i)} or {b.doc_stats(i)["lds_index"]}


@pytest.mark.parametrize("debug", ["0", "1"])
@pytest.mark.parametrize("staging", ["device", "host"])
def test_whole_documents(monkeypatch, docs, debug, staging):
    monkeypatch.setenv("DTGPU_DEBUG", debug)
    _, data, want = docs
    b = dt_amd.Batch(docs=data, staging=staging, flags=dt_amd.OPT_NO_SEGMENTS)
    assert _run(b, len(data)) == want
    assert all(b.segments(i) == [] and _tiers(b, i) == {1} for i in range(len(data)))


@pytest.mark.parametrize("debug", ["0", "1"])
def test_three_level_lds_tier(monkeypatch, docs, debug):
    """DTGPU_FLAT=0: the same documents on the 3-level LDS index, which the same routines serve."""
    monkeypatch.setenv("DTGPU_DEBUG", debug)
    monkeypatch.setenv("DTGPU_FLAT", "0")
    _, data, want = docs
    b = dt_amd.Batch(docs=data, staging="device", flags=dt_amd.OPT_NO_SEGMENTS)
    assert _run(b, len(data)) == want
    assert all(b.segments(i) == [] and _tiers(b, i) == {1} for i in range(len(data)))


@pytest.mark.parametrize("debug", ["0", "1"])
@pytest.mark.parametrize("staging", ["device", "host"])
def test_forced_segments(monkeypatch, docs, debug, staging):
    """Segments of four op runs and more: every later segment starts from placeholder items, whose
    ids follow the LVs.  Every document is cut.  A cut point needs every earlier op in the history
    of every later one, so `tie` and `passes` can be cut only after their concurrent branches: those
    corners run in a first segment, without placeholders, and the segments after it insert among
    placeholder items; `runs`, `boundary` and `delete` meet theirs in later segments."""
    monkeypatch.setenv("DTGPU_DEBUG", debug)
    monkeypatch.setenv("DTGPU_SEG_OPS", "4")
    names, data, want = docs
    b = dt_amd.Batch(docs=data, staging=staging)
    assert _run(b, len(data)) == want
    cut = {n: len(b.segments(i)) for i, n in enumerate(names)}
    assert all(k >= 2 for k in cut.values()), cut
    assert cut["runs"] >= 4 and cut["boundary"] >= 16, cut
    assert all(s["status"] == 0 for i in range(len(data)) for s in b.segments(i))


@pytest.mark.parametrize("debug", ["0", "1"])
def test_hbm_tier(monkeypatch, docs, debug):
    """An LDS index sized far too small (eight blocks): every document outgrows it and is replayed
    again, from its first command, on the HBM tier."""
    monkeypatch.setenv("DTGPU_DEBUG", debug)
    monkeypatch.setenv("DTGPU_LDS_FILL", "4000")
    names, data, want = docs
    b = dt_amd.Batch(docs=data, staging="device", flags=dt_amd.OPT_NO_SEGMENTS)
    assert _run(b, len(data)) == want
    assert [n for i, n in enumerate(names) if _tiers(b, i) != {0}] == []


def test_counters_of_the_paths(monkeypatch, docs):
    """DTGPU_DEBUG=2: skipped lookups, splits and dirty loads on the documents built for them."""
    monkeypatch.setenv("DTGPU_DEBUG", "2")
    names, data, want = docs
    b = dt_amd.Batch(docs=data, staging="device", flags=dt_amd.OPT_NO_SEGMENTS)
    assert _run(b, len(data)) == want
    st = {n: b.doc_stats(i) for i, n in enumerate(names)}
    assert st["fill"]["n_lookup_skip"] > 0 and st["fill"]["n_split"] > 0
    assert st["runs"]["n_split"] > 0 and st["boundary"]["n_lookup_skip"] > 0
    assert st["passes"]["n_dirty"] > 0 and st["tie"]["n_dirty"] > 0
