"""tests/lane_flag_docs.py on the CPU: every document's text through the host model of the tracker
(tools/poscache_model.py) is the oracle's, and the model, instrumented here, reaches the corners of
the replay's lane-flag handling each document is built for (dt_replay.hip F_LIVE / F_VIS)."""
import collections
import os
import sys

import pytest

import lane_flag_docs as D
from oracle.oracle import OpLog as OracleOpLog

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import poscache_model as M  # noqa: E402


class Probe(M.Model):
    """The model, counting the corners an edit takes."""

    def __init__(self, *a):
        super().__init__(*a)
        self.corners = collections.Counter()
        self._dropped = None     # the block a pass just dropped from the cache
        self._agent_calls = 0

    def insert_run(self, b, s, lv, k, ol, orr):
        c, n = self.corners, len(self.items[b])
        c[f"run_{k}"] += 1
        if n + k <= M.BLK:   # the run fits its block
            c["slot_0"] += s == 0 and n > 0
            c["slot_mid"] += 0 < s < n
            c["slot_last"] += s == M.BLK - 1
            c["fits_64"] += n + k == M.BLK
        c["split_65"] += n + k == M.BLK + 1
        c["orr_end"] += orr == M.END_ID
        c["orr_deleted"] += orr != M.END_ID and self.cnt[orr] >= 2
        super().insert_run(b, s, lv, k, ol, orr)

    def load(self, b):
        self.corners["dirty_reload_of_dropped"] += self.dirty[b] and b == self._dropped
        super().load(b)

    def do_insert(self, lv, k, pos):
        self.corners["pos_0"] += pos == 0
        emptied = self.stats["emptied_then_insert"]
        super().do_insert(lv, k, pos)
        self.corners["emptied_then_insert"] += self.stats["emptied_then_insert"] - emptied
        self._dropped = None

    def do_delete(self, lv, n, pos, fwd):
        rounds = self.stats["delete_rounds"]
        inside = self.find_vis(pos)[1] > 0   # the run starts past its block's first visible item
        super().do_delete(lv, n, pos, fwd)
        crossed = self.stats["delete_rounds"] - rounds > 1   # and runs on into the next block
        self.corners[f"del_{'fwd' if fwd else 'back'}_{n}"] += n == 1 or (crossed and inside)
        self._dropped = None

    def agent_of(self, lv):
        self._agent_calls += 1
        return super().agent_of(lv)

    def yjs_scan(self, *a):
        self._agent_calls = 0
        r = super().yjs_scan(*a)
        self.corners["yjs"] += 1
        self.corners["yjs_tie_by_agent"] += self._agent_calls > 1   # past the new item's own lookup
        return r

    def toggle(self, off, n):
        cb = self.cb
        super().toggle(off, n)
        self.corners[f"pass_{n}"] += 1
        if cb is not None and self.cb is None:
            self._dropped = cb


WANT = {
    "fill": ("slot_0", "slot_last", "slot_mid", "fits_64", "split_65", "orr_end"),
    "runs": tuple(f"run_{k}" for k in D.RUNS) + ("pos_0", "orr_end", "slot_mid"),
    "boundary": ("orr_deleted", "emptied_then_insert", "del_fwd_130"),
    # (a backspace run of one character is a forward run of one: the plan has no direction for it)
    "delete": ("del_fwd_1", "del_fwd_64", "del_fwd_130", "del_back_64", "del_back_130"),
    "tie": ("yjs_tie_by_agent", "orr_end", "orr_deleted"),
    "passes": ("pass_1", "pass_64", "dirty_reload_of_dropped"),
}


@pytest.fixture(scope="module")
def docs():
    return D.all_docs()


@pytest.fixture(scope="module")
def models(docs):
    out = {}
    for name, o in docs.items():
        m = Probe(o.plan_commands(), o.plan_tlist(), o.agent_runs(), len(o))
        m.run()
        out[name] = m
    return out


@pytest.mark.parametrize("name", list(D.BUILDERS))
def test_model_text_is_the_oracles(docs, models, name):
    o = docs[name]
    assert len(o) <= 5000
    assert models[name].stats["disagree"] == 0
    assert M.text_of(o, models[name]) == OracleOpLog.load_from(o.encode()).checkout_tip_bytes()


@pytest.mark.parametrize("name", list(D.BUILDERS))
def test_document_reaches_its_corners(models, name):
    c = models[name].corners
    assert all(c[k] > 0 for k in WANT[name]), {k: c[k] for k in WANT[name]}


def test_counters_the_gpu_test_expects_are_nonzero(models):
    """tests/test_gpu_lane_flags.py asserts these of the instrumented kernel (DTGPU_DEBUG=2)."""
    assert models["fill"].stats["skips"] > 0 and models["fill"].stats["splits"] > 0
    assert models["runs"].stats["splits"] > 0
    assert models["boundary"].stats["skips"] > 0
    assert models["passes"].stats["dirty_loads"] > 0 and models["tie"].stats["dirty_loads"] > 0
