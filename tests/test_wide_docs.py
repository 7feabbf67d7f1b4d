"""CPU checks of the fan generator (wide_docs.py) and of the host code at the 64-lane widths: the
documents have the structure the GPU tests rely on (a frontier, a parent list and retreat / advance
passes of exactly 63, 64 and 65), the oracle converges on them and equals the plain models, and
the host's history / encode_from / decode_and_add / dominators hold at a version W - 1 wide."""
import numpy as np
import pytest

import wide_docs as W
from oracle.oracle import OpLog as OracleOpLog
import dt_amd

SINGLE = [("del_same",), ("del_same2",), ("ins_same",)]


def _loaded(o):
    return dt_amd.ListOpLog.load_from(o.encode())


def _parent_counts(o):
    po = o.export("parent_offsets")
    return [int(po[k + 1] - po[k]) for k in range(len(po) - 1)]


@pytest.mark.parametrize("width", W.WIDTHS)
def test_structure(width):
    o = _loaded(W.fan(width))
    assert len(o.local_frontier()) == width
    assert len(o) == 10 + 5 * width
    assert len(o.export("agent_names")) == width + 1
    m = _loaded(W.fan(width, merge=True))
    assert max(_parent_counts(m)) == (width if width >= 2 else 0)   # (a 1-fan is one linear entry)
    assert len(m) == 10 + 5 * width + W.merge_tail_chars(width)
    if width >= 4:   # the second wide merge
        assert sorted(_parent_counts(m))[-2:] == [width // 2, width]
    # the interleaved build is the same document once it went through a file
    il = _loaded(W.fan(width, merge=True, interleave=True))
    for what in ("entries", "parents", "parent_offsets", "ops", "agent_runs"):
        assert np.array_equal(il.export(what), m.export(what)), what


def test_names_differ_from_id_order():
    names = W.agent_names(96)
    assert len(set(names)) == 96
    by_name = sorted(range(8), key=lambda i: W.agent_names(8)[i])
    assert "".join("ABCDEFGH"[i] for i in by_name) == "ADGBEHCF"
    assert sorted(W.agent_names(8)) == ["w005", "w015", "w025", "w042", "w052", "w062", "w079", "w089"]


@pytest.mark.parametrize("width", W.WIDTHS)
def test_oracle_converges_and_equals_the_models(width):
    for merge in (False, True):
        ora = OracleOpLog.load_from(W.fan(width, merge=merge).encode())
        t = ora.checkout_tip_bytes(order=0)
        assert t == ora.checkout_tip_bytes(order=1)
        assert len(t.decode()) == W.mixed_char_count(width, merge), merge
    for shape in SINGLE:
        ora = OracleOpLog.load_from(W.fan(width, shape).encode())
        t = ora.checkout_tip_bytes(order=0)
        assert t == ora.checkout_tip_bytes(order=1), shape
        assert t.decode() == W.model_text(width, shape), shape
        m = OracleOpLog.load_from(W.fan(width, shape, merge=True).encode())
        assert m.checkout_tip_bytes(order=0) == m.checkout_tip_bytes(order=1), shape


def test_models_by_hand():
    assert W.model_text(64, ("del_same",)) == "013456789"
    assert W.model_text(64, ("del_same2",)) == "01456789"
    assert W.model_text(3, ("ins_same",)) == "01234" + chr(0x100) + chr(0x101) + chr(0x102) + "56789"   # w005 w042 w079
    assert W.model_text(4, ("ins_same",))[5:9] == chr(0x100) + chr(0x103) + chr(0x101) + chr(0x102)     # w015 is branch 3
    assert len(W.branch_char(95).encode()) == 2


@pytest.mark.parametrize("width", W.WIDTHS)
def test_host_round_trip_at_a_wide_version(width):
    o = _loaded(W.fan(width))
    fr = o.local_frontier()
    assert o.dominators(range(len(o))) == fr
    v = fr[:max(1, width - 1)]
    sub = o.history(v)
    assert len(sub) == len(o) - (5 if width >= 2 else 0)
    sub.decode_and_add(o.encode_from(v, dt_amd.ENCODE_PATCH))
    assert len(sub) == len(o)
    assert len(sub.local_frontier()) == width


@pytest.mark.parametrize("width,k", [(2, 4), (8, 3), (17, 4), (64, 4), (65, 3)])
def test_parts_keep_the_interleaved_lv_order(width, k):
    built, part, patches = W.as_parts(width, k=k)
    assert len(patches) == 3 * -(-width // k)
    host = dt_amd.ListOpLog.load_from(part)
    for p in patches:
        host.decode_and_add(p)
    for what in ("entries", "parents", "parent_offsets", "ops", "agent_runs", "version"):
        assert np.array_equal(host.export(what), built.export(what)), what
    if width >= 2:   # interleaved: an entry per step, not per branch
        assert len(built.export("entries")) > 2 * width
    want = OracleOpLog.load_from(W.fan(width).encode()).checkout_tip_bytes()
    assert OracleOpLog.load_from(built.encode()).checkout_tip_bytes() == want


def _applied(part, patches):
    host = dt_amd.ListOpLog.load_from(part)
    for p in patches:
        host.decode_and_add(p)
    return host


def _same_document(a, b):
    """The same operations, whatever the LV order (a part is a file: written in walk order)."""
    assert len(a) == len(b) and len(a.local_frontier()) == len(b.local_frontier())
    ta, tb = (OracleOpLog.load_from(x.encode()).checkout_tip_bytes() for x in (a, b))
    assert ta == tb


@pytest.mark.parametrize("width,extra,merge", [(60, 3, False), (60, 4, False), (60, 5, False),
                                               (63, 0, True), (64, 0, True), (65, 0, True)])
def test_grown_fans(width, extra, merge):
    built, part, patch = W.grown(width, extra, merge=merge)
    host = _applied(part, [patch])
    _same_document(host, built)
    assert len(dt_amd.ListOpLog.load_from(part).local_frontier()) == width
    if merge:
        assert max(_parent_counts(host)) == width and W.widest_frontier(host) == width
    else:
        assert len(host.local_frontier()) == width + extra == W.widest_frontier(host)


@pytest.mark.parametrize("width", [64, 66, 96])
def test_halves_hold_a_wide_version_under_a_narrow_frontier(width):
    built, part, patch = W.halves(width)
    host = _applied(part, [patch])
    _same_document(host, built)
    tips = W.branch_tips(host)
    assert W.widest_frontier(host) == width - width // 2 + 1 <= 64
    assert len(tips) == width and host.dominators(tips) == tips
    assert host.dominators(range(len(host))) == host.local_frontier()
    assert len(host.local_frontier()) == width - width // 2 + 1
    for k in (63, 64, 65):
        if k <= width:
            assert len(host.history(tips[:k])) == 10 + 5 * k


def test_inputs_cover_the_one_chunk_pass_boundary():
    """From the host planner: all-delete passes of exactly 63, 64 and 65 entries on one item (the
    single-LV delete shape's final pass has W - 1 entries), the two-LV form's 64 entries at 33
    branches (under 64 chains), and passes of 63, 64 and 65 sibling inserts at one position -- so a
    generator change cannot silently empty a case."""
    for width in (64, 65, 66):
        for shape, dels in ((("del_same",), width - 1), (("ins_same",), 0)):
            passes = W.toggle_passes(_loaded(W.fan(width, shape)))
            assert passes[-1] == (width - 1, dels), (width, shape)
            assert max(n for n, _ in passes) == width - 1
    passes = W.toggle_passes(_loaded(W.fan(33, ("del_same2",))))
    assert passes[-1] == (64, 64)
    # the mixed shape's passes lie on both sides of the dispatch and mix kinds
    passes = W.toggle_passes(_loaded(W.fan(65, merge=True)))
    assert any(n <= 64 for n, _ in passes) and any(n > 128 for n, _ in passes)
    assert any(0 < k < n for n, k in passes)
