"""The flat-tier replay's position cache (dt_replay.hip D.cpre / cpos: an edit that lands among the
visible items of the block cached in registers skips the index scan).  Every invariant case runs
the instrumented kernel (DTGPU_DEBUG=1), which after every command recomputes the cached block's
position and visible prefix from the index, and compares the text with the oracle's or the golden
one.  The counter cases (DTGPU_DEBUG=2) compare the kernel's lookup / skipped-lookup counts with
tools/poscache_model.py's, exactly.  The other tiers and modes, which never skip, keep their texts."""
import os
import sys

import pytest

import golden_data as G
import poscache_docs as P
import wide_docs as W
from oracle.oracle import OpLog as OracleOpLog

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

import dt_amd  # noqa: E402
import poscache_model as M  # noqa: E402

N_MERGE, N_EPOCH, N_OPS = 32, 8, 5000


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if dt_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the engine has no CPU fallback")


def _oracle(data):
    return OracleOpLog.load_from(data).checkout_tip_bytes()


def _ff_want():
    return G.trace("friendsforever_flat")["endContent"].encode()


@pytest.fixture(scope="module")
def synth():
    """(oplogs, .dt bytes, oracle texts) of the 32 pairwise-merge documents and 8 of the epoch family."""
    oplogs = [dt_amd.synth_merge_oplog(d, N_OPS) for d in range(N_MERGE)] + \
             [dt_amd.synth_oplog(d, N_OPS) for d in range(N_EPOCH)]
    docs = [o.encode() for o in oplogs]
    return oplogs, docs, [_oracle(d) for d in docs]


@pytest.fixture(scope="module")
def two_agent():
    data = P.two_agent_doc().encode()
    return data, _oracle(data)


def _run(b, n):
    b.run()
    b.sync()
    res = b.results()
    assert [r["status"] for r in res] == [0] * n, [(i, r, b.doc_stats(i)) for i, r in enumerate(res) if r["status"]]
    return [b.text(i) for i in range(n)]


def _tiers(b, i):
    return {s["lds_index"] for s in b.segments(i)} or {b.doc_stats(i)["lds_index"]}


# ---- invariants and texts (DTGPU_DEBUG=1) -----------------------------------------------------------

def test_friendsforever_alone_as_segments(monkeypatch):
    """Alone the document is cut into segments: the cache over placeholder blocks."""
    monkeypatch.setenv("DTGPU_DEBUG", "1")
    b = dt_amd.Batch(docs=[G.dt_bytes("friendsforever")], staging="device")
    texts = _run(b, 1)
    assert len(b.segments(0)) >= 2 and all(s["status"] == 0 for s in b.segments(0))
    assert _tiers(b, 0) == {1}
    assert texts[0] == _ff_want()


def test_synthetic_documents_in_one_batch(monkeypatch, synth):
    monkeypatch.setenv("DTGPU_DEBUG", "1")
    _, docs, want = synth
    b = dt_amd.Batch(docs=docs, staging="device")
    assert _run(b, len(docs)) == want
    assert all(_tiers(b, i) == {1} for i in range(len(docs)))


def test_passes_of_63_64_and_65_entries_on_one_item(monkeypatch):
    """The fans of 63, 64 and 65, and of 66: a w-fan's single-op shapes end in one pass of w - 1
    entries on one item (62 to 65: toggle_pass_1 up to 64 entries, toggle_pass above), the merged
    mixed fans have passes of some 160 (host-staged: a fan past 64 has more chains than the device
    staging takes)."""
    monkeypatch.setenv("DTGPU_DEBUG", "1")
    widths = (63, 64, 65, 66)
    oplogs = [W.fan(w, s) for w in widths for s in (("del_same",), ("ins_same",))]
    oplogs += [W.fan(w, merge=True, interleave=True) for w in widths]
    widest = [max(n for n, _ in W.toggle_passes(o)) for o in oplogs[:8:2]]
    assert widest == [62, 63, 64, 65], widest
    b = dt_amd.Batch(oplogs=oplogs)
    assert _run(b, len(oplogs)) == [_oracle(o.encode()) for o in oplogs]
    assert all(_tiers(b, i) == {1} for i in range(len(oplogs)))


def test_two_agent_document(monkeypatch, two_agent):
    """tests/poscache_docs.py; tests/test_poscache_model.py asserts the corners it reaches."""
    monkeypatch.setenv("DTGPU_DEBUG", "1")
    data, want = two_agent
    b = dt_amd.Batch(docs=[data], staging="device", flags=dt_amd.OPT_NO_SEGMENTS)
    assert _run(b, 1) == [want]
    assert b.segments(0) == [] and b.doc_stats(0)["lds_index"] == 1 and b.doc_stats(0)["n_blocks"] > 64


# ---- counters (DTGPU_DEBUG=2) ---------------------------------------------------------------------

def _counters(monkeypatch, data):
    monkeypatch.setenv("DTGPU_DEBUG", "2")
    b = dt_amd.Batch(docs=[data], staging="device", flags=dt_amd.OPT_NO_SEGMENTS)
    text = _run(b, 1)[0]
    st = b.doc_stats(0)
    assert b.segments(0) == [] and st["lds_index"] == 1
    m = M.model_oplog(dt_amd.ListOpLog.load_from(data))
    assert m.stats["disagree"] == 0
    return text, st, m.stats


def test_friendsforever_counters_equal_the_model(monkeypatch):
    text, st, want = _counters(monkeypatch, G.dt_bytes("friendsforever"))
    assert text == _ff_want()
    assert (want["lookups"], want["skips"]) == (4097, 2252)
    assert (st["n_lookup"], st["n_lookup_skip"]) == (want["lookups"], want["skips"])
    assert (st["n_blocks"], st["n_split"], st["n_dirty"]) == (want["blocks"], want["splits"], want["dirty_loads"])


def test_two_agent_counters_equal_the_model(monkeypatch, two_agent):
    data, text_want = two_agent
    text, st, want = _counters(monkeypatch, data)
    assert text == text_want
    assert (st["n_lookup"], st["n_lookup_skip"]) == (want["lookups"], want["skips"])
    assert (st["n_blocks"], st["n_split"]) == (want["blocks"], want["splits"])


# ---- the paths that keep calling find_vis ---------------------------------------------------------

def test_host_staged_batch(synth):
    oplogs, _, want = synth
    b = dt_amd.Batch(oplogs=oplogs[:8] + oplogs[N_MERGE:N_MERGE + 2])
    assert _run(b, 10) == want[:8] + want[N_MERGE:N_MERGE + 2]


def test_hbm_tier_batch(monkeypatch, synth):
    """An LDS index sized far too small (8 blocks): the documents hand back to the HBM tier."""
    monkeypatch.setenv("DTGPU_LDS_FILL", "4000")
    _, docs, want = synth
    b = dt_amd.Batch(docs=docs[:4], staging="device")
    assert _run(b, 4) == want[:4]
    assert all(_tiers(b, i) == {0} for i in range(4))


def test_transformed_ops_of_resident_documents(synth):
    oplogs, docs, want = synth
    pick = [0, 1, N_MERGE]
    d = dt_amd.DecodeBatch([docs[k] for k in pick])
    d.run()
    hosts = [dt_amd.ListOpLog.load_from(docs[k]) for k in pick]
    m = d.xf_operations_from(range(len(pick)), [[]] * len(pick), [h.local_frontier() for h in hosts])
    for i, k in enumerate(pick):
        assert m.status(i) == 0
        assert m.xf_operations_lv(i) == hosts[i].xf_operations_lv()
        assert m.content_bytes(i) == want[k]
