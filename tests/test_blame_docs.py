"""The blame model of tests/blame_docs.py, pinned on the CPU before the GPU is asked anything: for
every builder document the model's list of LVs, read as characters, is the oracle's checkout, and
the runs have the properties the blame is defined by."""
import pytest

import blame_docs as BD
import golden_data as G
import linear_docs
import merge_docs
from oracle.oracle import OpLog as OracleOpLog

DOCS = BD.small_docs()


def _check_runs(ora, version=None):
    lvs = BD.model_lvs(ora, version)
    want = ora.checkout_tip_bytes() if version is None else ora.checkout_bytes(list(version))
    assert BD.lv_text(ora, lvs) == want
    runs = BD.model_runs(ora, version)
    assert sum(r[1] for r in runs) == len(lvs) == len(want.decode())
    flat = [lv + k for lv, n, _a, _s in runs for k in range(n)]
    assert flat == lvs
    for x, y in zip(runs, runs[1:]):   # maximal: two adjacent runs never merge
        assert not (x[0] + x[1] == y[0] and x[2] == y[2] and x[3] + x[1] == y[3])
    return runs


@pytest.mark.parametrize("name", sorted(DOCS))
def test_model_text_is_the_oracles(name):
    _check_runs(OracleOpLog.load_from(DOCS[name]))


def test_known_run_counts():
    n = {k: len(BD.model_runs(OracleOpLog.load_from(DOCS[k]))) for k in DOCS}
    assert n["deleted_middle"] == 2 and n["insert_in_middle"] == 3 and n["insert_deleted_again"] == 1
    assert n["all_deleted"] == 0 and n["all_deleted_concurrently"] == 0 and n["no_inserts"] == 0
    assert n["agent_boundary"] == 2 and n["tie_break"] == 3
    for w in BD.WIDTHS:
        assert n[f"one_run_{w}"] == 1 and n[f"alternating_{w}"] == w
    # the linear turns: the first piece of the final text spans more than two agent runs
    ora = OracleOpLog.load_from(DOCS["linear_turns"])
    first = BD.lv_runs(BD.model_lvs(ora))[0]
    agents = {r[2] for r in BD.model_runs(ora) if first[0] <= r[0] < first[0] + first[1]}
    inside = [r for r in BD.model_runs(ora) if first[0] <= r[0] < first[0] + first[1]]
    assert len(inside) > 2 and agents == {"ann", "bob"}


def test_friendsforever_model():
    ora = OracleOpLog.load_from(G.dt_bytes("friendsforever"))
    lvs = BD.model_lvs(ora)
    assert len(lvs) == 21362 and len(BD.lv_runs(lvs)) == 2436
    assert BD.lv_text(ora, lvs) == ora.checkout_tip_bytes()


@pytest.mark.parametrize("seed", [1, 2])
def test_linear_builders(seed):
    data, want = linear_docs.random_linear(seed, 150)
    ora = OracleOpLog.load_from(data)
    assert BD.lv_text(ora, BD.model_lvs(ora)) == want
    data, want = linear_docs.sized_linear(130, seed)
    ora = OracleOpLog.load_from(data)
    assert BD.lv_text(ora, BD.model_lvs(ora)) == want


def test_two_blocks_and_versions():
    _check_runs(OracleOpLog.load_from(BD.two_blocks(3000)))
    data = merge_docs.small_bytes()
    ora = OracleOpLog.load_from(data)
    import dt_amd
    for v in merge_docs.versions(dt_amd.ListOpLog.load_from(data)):
        _check_runs(ora, v)
