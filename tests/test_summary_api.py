"""Version summaries on the host: `ListOpLog.summarize_versions` / `intersect_with_summary`
(dtgpu_oplog_summarize, dtgpu_oplog_intersect_summary) against the reference's own vectors
(src/causalgraph/summary.rs `summary_smoke`, `intersect_summary`, expected values written here as
data) and against tests/summary_model.py, a plain restatement of summary.rs.  No GPU needed: these
functions are what the batched device calls are compared with (test_gpu_summary.py)."""
import random

import pytest

import golden_data as G
import summary_docs as D
import summary_model as M
import dt_amd


def _norm(summary):
    return dt_amd.normalize_summary(summary)


def _model(o, summary, frontier=()):
    doc, sm = M.Doc(o), _norm(summary)
    f, rec = M.intersect(doc, sm, frontier)
    return f, rec, M.group(sm, rec)


def _same_as_model(o, summary, frontier=()):
    f, rec, grouped = _model(o, summary, frontier)
    st, hf, hrec = o.intersect_summary_records(summary, frontier)
    assert (st, hf, hrec) == (0, f, rec), (summary, frontier)
    assert o.intersect_with_summary(summary, frontier) == (f, grouped)
    return f, grouped


def test_summary_smoke():
    """summary.rs:297-373."""
    o = dt_amd.ListOpLog()
    assert o.summarize_versions() == []
    o.get_or_create_agent_id("seph")
    o.get_or_create_agent_id("mike")
    assert o.summarize_versions() == []   # agents without ops are omitted
    o.add_insert_at(0, [], 0, "a" * 5)
    assert o.summarize_versions() == [("seph", [(0, 5)])]
    before, after = D.smoke_doc()
    assert before.summarize_versions() == [("seph", [(0, 10)]), ("mike", [(0, 5)])]
    assert after.summarize_versions() == [("seph", [(0, 10)]), ("mike", [(0, 5), (15, 20)])]
    for o in (before, after):
        assert [(n.decode(), r) for n, r in M.summarize(M.Doc(o))] == o.summarize_versions()
    # the flat form [(name, next_seq)] stands for name: [(0, next_seq)]
    assert before.intersect_with_summary([("seph", 10), ("mike", 5)], [9]) == ([9, 14], None)
    assert before.intersect_with_summary([("seph", 10), ("mike", 5)], [9]) == \
        before.intersect_with_summary([("seph", [(0, 10)]), ("mike", [(0, 5)])], [9])


def test_intersect_summary_reference_vectors():
    """summary.rs:410-481."""
    empty = dt_amd.ListOpLog()
    empty.get_or_create_agent_id("seph")
    assert empty.intersect_with_summary(D.REF_VS) == ([], D.REF_VS)          # :434-436
    o = D.sparse_doc()
    assert o.summarize_versions() == [("seph", [(1, 5), (8, 9)])]
    # intersect_with_summary_full's visits (:452-459): (name, range, base LV)
    assert M.pieces(M.Doc(o), _norm(D.REF_VS)) == [
        (0, 0, 1, None), (0, 1, 5, 0), (0, 5, 8, None), (0, 8, 9, 4), (0, 9, 10, None), (1, 0, 5, None)]
    want = ([3, 4], [("seph", [(0, 1), (5, 8), (9, 10)]), ("mike", [(0, 5)])])   # :461-472
    assert o.intersect_with_summary(D.REF_VS) == want
    assert _same_as_model(o, D.REF_VS) == want
    o, v = D.sparse_doc_with_kaarina()
    assert o.intersect_with_summary(D.REF_VS, [v])[0] == [v]                 # :474-480: [v] dominates
    _same_as_model(o, D.REF_VS, [v])


def test_statuses_and_edges():
    o = D.sparse_doc()
    assert o.intersect_with_summary([]) == ([], None)                         # ROOT
    assert o.intersect_with_summary([], [2]) == ([2], None)
    for bad in ([("seph", [(3, 3)])], [("seph", [(5, 2)])], [("nobody", [(0, 0)])]):
        with pytest.raises(dt_amd.ParseError) as e:
            o.intersect_with_summary(bad)
        assert e.value.code == 67
    with pytest.raises(dt_amd.ParseError) as e:
        o.intersect_with_summary(D.REF_VS, [len(o)])
    assert e.value.code == 67
    # bounds far past the document come back unchanged; unknown pieces are never merged across ranges
    far = [("seph", [(0, 1), (4, 9), (9, 1 << 40), (1 << 40, (1 << 40) + 7)]), ("ROOT", [(0, 3)]), ("seph", [(9, 12)])]
    assert o.intersect_with_summary(far) == (
        [3, 4], [("seph", [(0, 1), (5, 8), (9, 1 << 40), (1 << 40, (1 << 40) + 7)]), ("ROOT", [(0, 3)]),
                 ("seph", [(9, 12)])])
    _same_as_model(o, far)
    # only the last LV of a clipped piece counts: seph 1..3 is LVs 0..1
    assert o.intersect_with_summary([("seph", [(1, 3)])]) == ([1], None)
    # a remote frontier is unit ranges; one this oplog lacks raises
    assert o.remote_frontier_to_local([("seph", 4), ("seph", 8)]) == [3, 4]
    with pytest.raises(KeyError):
        o.remote_frontier_to_local([("seph", 6)])


def test_runs_out_of_seq_order():
    for sparse in (False, True):
        o = D.reordered_host(sparse)
        want = [("x", [(0, 5), (10, 15)] if sparse else [(0, 10)]), ("y", [(0, 2)])]
        assert o.summarize_versions() == want
        assert [(n.decode(), r) for n, r in M.summarize(M.Doc(o))] == want
        f, rem = _same_as_model(o, [("x", [(2, 13)]), ("x", [(0, 20)])])
        assert f == [4, 11]   # the last LV of each span of x; y is not in the summary
        assert rem == [("x", [(5, 10), (5, 10), (15, 20)] if sparse else [(10, 13), (10, 20)])]


@pytest.mark.parametrize("seed", range(4))
def test_random_documents_against_the_model(seed):
    rng = random.Random(1000 + seed)
    o = dt_amd.synth_merge_oplog(seed, 250)
    assert [(n.decode(), r) for n, r in M.summarize(M.Doc(o))] == o.summarize_versions()
    for _ in range(40):
        _same_as_model(o, D.random_summary(rng, o), D.random_frontier(rng, o))
    _same_as_model(o, [])
    _same_as_model(o, o.summarize_versions())


def test_friendsforever_round_trip():
    o = dt_amd.ListOpLog.load_from(G.dt_bytes("friendsforever"))
    mine = o.summarize_versions()
    rng = random.Random(7)
    for v in [0, len(o) - 1] + [rng.randrange(len(o)) for _ in range(6)]:
        c = o.history([v])
        assert o.intersect_with_summary(c.summarize_versions()) == (o.dominators([v]), None)
        f, rem = c.intersect_with_summary(mine)
        assert f == c.local_frontier()
        assert sum(e - s for _n, rs in (rem or []) for s, e in rs) == len(o) - len(c)
