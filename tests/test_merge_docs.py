"""The small merge document (tests/merge_docs.py) on the CPU: what it is, and -- with the oracle
alone -- that for all 1,444 ordered pairs of its 38 versions the transformed stream applied to the
checkout at `from` gives the checkout at the merged frontier; the host walk order equals the
oracle's for every pair.  tests/test_gpu_merge.py sends the same pairs to the device."""
from oracle.oracle import OpLog as OracleOpLog
import dt_amd

import merge_docs as M


def _loaded():
    data = M.small_bytes()
    return dt_amd.ListOpLog.load_from(data), OracleOpLog.load_from(data)


def test_small_document_is_what_the_tests_rely_on():
    o, ora = _loaded()
    assert len(o) == 15
    assert len(M.small().export("entries")) == 6   # as built; the file joins each branch's two entries
    assert len(o.export("entries")) == 4
    assert len(o.export("agent_names")) == 3
    assert ora.checkout_tip_bytes().decode() == M.SMALL_TEXT
    vs = M.versions(o)
    assert len(vs) == 38 and sum(len(v) == 2 for v in vs) == 22
    assert len(M.all_pairs(o)) == 1444
    # a three-parent merge entry
    po = o.export("parent_offsets")
    assert max(int(po[k + 1]) - int(po[k]) for k in range(len(po) - 1)) == 3


def test_oracle_stream_takes_from_to_the_merged_checkout_for_every_pair():
    o, ora = _loaded()
    ex = M.exports(o)
    already = 0
    for a, b in M.all_pairs(o):
        stream = ora.xf_operations_from(a, b)
        already += sum(1 for _lv, x in stream if x < 0)
        got = M.apply(ora.checkout_bytes(a).decode(), M.per_char(ex, stream))
        assert got == ora.checkout_bytes(o.dominators(a, b)).decode(), (a, b)
    assert already == 245   # DeleteAlreadyHappened records over all pairs


def test_host_xf_order_matches_oracle_for_every_pair():
    o, ora = _loaded()
    for a, b in M.all_pairs(o):
        assert o.xf_order(a, b) == [lv for lv, _ in ora.xf_operations_from(a, b)], (a, b)


def test_merge_xf_runs_is_the_generator_iter_xf_operations_uses():
    """The run-merging as a module function over (ops, content, char_offsets, stream): an insert
    run, a forward delete and a DeleteAlreadyHappened record."""
    o, _ = _loaded()
    ops, content, coff = M.exports(o)
    n = len(o)
    first = [int(ops[0][0]) + k for k in range(int(ops[0][1]))]
    stream = [(lv, k) for k, lv in enumerate(first)]
    out = list(dt_amd.merge_xf_runs(ops, content, coff, stream))
    assert len(out) == 1 and out[0][0] == range(first[0], first[-1] + 1)
    assert out[0][1][0] == "ins" and out[0][1][1] == 0 and len(out[0][1][2]) == len(first)
    dels = [int(lv) for lv, ln, _p, kf in ops if int(kf) & 1 for _ in range(1)]
    assert dels and dels[0] < n
    assert list(dt_amd.merge_xf_runs(ops, content, coff, [(dels[0], None)])) == [(range(dels[0], dels[0] + 1), None)]
