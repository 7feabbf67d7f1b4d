"""The replay's one-chunk retreat / advance pass (dt_replay.hip toggle_pass_1: passes of at most 64
entries, as straight-line code) beside the chunked pass it dispatches from: 64 small synthetic
documents whose passes lie on both sides of the dispatch and on its boundary, with no, few and
many delete entries, replayed on the flat LDS tier, the 3-level LDS tier and the HBM tier, with
the debug invariant checks after every command, plus the golden friendsforever document (whole,
and alone as segments) and a linear backspace trace kept on the tracker.  Every text must equal
the CPU oracle's / the golden text."""
import pytest

import golden_data as G
from oracle.oracle import OpLog as OracleOpLog

pytestmark = pytest.mark.gpu

import dt_amd  # noqa: E402

SEEDS = range(32)
N_OPS = 400
# The hand-back to the HBM tier needs documents that outgrow the smallest LDS index the layout ever
# reserves (8 blocks = 512 items): 3,000 LVs hold about 1,200 inserted items, 19 full blocks at least.
BIG_SEEDS = range(4)
BIG_OPS = 3000
N_SMALL = 2 * len(SEEDS)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if dt_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the engine has no CPU fallback")


@pytest.fixture(scope="module")
def docs():
    return ([dt_amd.synth_merge_oplog(d, N_OPS).encode() for d in SEEDS]
            + [dt_amd.synth_oplog(d, N_OPS).encode() for d in SEEDS]
            + [dt_amd.synth_merge_oplog(d, BIG_OPS).encode() for d in BIG_SEEDS]
            + [dt_amd.synth_oplog(d, BIG_OPS).encode() for d in BIG_SEEDS])


@pytest.fixture(scope="module")
def want(docs):
    return [OracleOpLog.load_from(d).checkout_tip_bytes() for d in docs]


def _ff_want():
    return G.trace("friendsforever_flat")["endContent"].encode()


def _run(docs):
    b = dt_amd.Batch(docs=docs, staging="device")
    b.run()
    b.sync()
    res = b.results()
    assert [r["status"] for r in res] == [0] * len(docs), [(i, r) for i, r in enumerate(res) if r["status"]]
    return b, [b.text(i) for i in range(len(docs))], [(r["text_len"], r["text_hash"]) for r in res]


def _tiers(b, i):
    """Where document i replayed (1: an LDS index, 0: the HBM index), over its segments if it was cut."""
    return {s["lds_index"] for s in b.segments(i)} or {b.doc_stats(i)["lds_index"]}


@pytest.fixture(scope="module")
def flat(docs):
    """The synthetic documents on the default (flat LDS) tier."""
    b, texts, recs = _run(docs)
    assert all(_tiers(b, i) == {1} for i in range(len(texts)))
    return texts, recs


def test_inputs_cover_both_paths_and_the_boundary(docs):
    """From the host planner (the device plan is tested equal to it): passes in every length band
    around the 64-entry dispatch, passes without, with few and with many delete entries, and
    delete runs in both orders -- so a generator change cannot silently empty a case."""
    lens, dels, runs = [], [], []
    for d in docs[:N_SMALL]:
        o = dt_amd.ListOpLog.load_from(d)
        cmds, tl = o.plan_commands(), o.plan_tlist()
        for op, a, n, _pos in cmds:
            if (op & 15) == 2:
                lens.append(n)
                dels.append(sum((e >> 30) & 1 for e in tl[a:a + n]))
            elif (op & 15) == 1:
                runs.append((n, bool(op & 16)))
    assert any(n <= 64 for n in lens)
    assert any(n == 64 for n in lens)
    assert any(n == 65 for n in lens)
    assert any(65 <= n <= 128 for n in lens)
    assert any(n > 128 for n in lens)
    short = [k for n, k in zip(lens, dels) if n <= 64]
    assert any(k == 0 for k in short) and any(1 <= k <= 4 for k in short) and any(k > 4 for k in short)
    assert any(k > 4 for k in dels)
    assert any(n >= 2 and fwd for n, fwd in runs) and any(n >= 2 and not fwd for n, fwd in runs)
    for d in docs[N_SMALL:]:   # the documents the HBM tier replays: both sides of the dispatch each
        o = dt_amd.ListOpLog.load_from(d)
        big = [n for op, _a, n, _pos in o.plan_commands() if (op & 15) == 2]
        assert any(n <= 64 for n in big) and any(n > 64 for n in big)


def test_flat_tier_matches_the_oracle(flat, want):
    texts, _ = flat
    assert texts == want


@pytest.mark.parametrize("env,lds", [({"DTGPU_FLAT": "0"}, 1), ({"DTGPU_LDS_FILL": "4000"}, 0)],
                         ids=["lds3", "hbm_handback"])
def test_other_tiers_match_the_flat_tier(monkeypatch, docs, flat, env, lds):
    """The 3-level LDS index, and an LDS index sized far too small (8 blocks): the 3,000-LV
    documents outgrow it and replay again on the HBM tier."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    b, texts, recs = _run(docs)
    assert (texts, recs) == flat
    tiers = [_tiers(b, i) for i in range(len(texts))]
    if lds:
        assert all(t == {1} for t in tiers)
    else:
        assert all(t == {0} for t in tiers[N_SMALL:])


def test_invariants_hold_after_every_command(monkeypatch, docs, flat):
    """The instrumented kernel (DTGPU_DEBUG=1) checks the whole index after every command."""
    monkeypatch.setenv("DTGPU_DEBUG", "1")
    _, texts, recs = _run(docs[:N_SMALL])
    assert (texts, recs) == (flat[0][:N_SMALL], flat[1][:N_SMALL])


@pytest.mark.parametrize("env,tiers", [({}, {1}), ({"DTGPU_FLAT": "0"}, {1}), ({"DTGPU_LDS_FILL": "4000"}, {0, 1})],
                         ids=["flat", "lds3", "hbm_handback"])
def test_friendsforever_alone_replays_as_segments(monkeypatch, env, tiers):
    """Alone, the document is cut into segments: each segment's passes (all of at most 64 entries)
    take the short path too; with the LDS index sized too small its later segments hand back."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    b, texts, _ = _run([G.dt_bytes("friendsforever")])
    assert len(b.segments(0)) >= 2 and all(s["status"] == 0 for s in b.segments(0))
    assert _tiers(b, 0) == tiers
    assert texts[0] == _ff_want()


def test_backspace_trace_on_the_tracker(monkeypatch):
    """A linear trace with backspace runs (reversed delete order), kept off the fast-forward path."""
    o = dt_amd.apply_edits_push_merge(G.trace("friendsforever_flat")["txns"])
    assert any((op & 15) == 1 and not (op & 16) and n >= 2 for op, _a, n, _pos in o.plan_commands())
    monkeypatch.setenv("DTGPU_FF", "0")
    b = dt_amd.Batch(docs=[o.encode()], staging="device")
    assert b.fast_forwarded() == [0]
    b.run()
    b.sync()
    assert b.results()[0]["status"] == 0
    assert b.text(0) == _ff_want()
