"""tools/poscache_model.py, the CPU model of the flat-tier replay's position cache: the host plan
replayed through 64-slot blocks with the one-block register cache and the cached-prefix rule the
kernel ships (dt_replay.hip D.cpre / cpos).  The model's text is the golden / the oracle's, the
prefix test never disagrees with the full lookup, and the friendsforever counts are pinned: they
are what tests/test_gpu_poscache.py expects of the instrumented kernel's counters."""
import os
import sys

import pytest

import golden_data as G
import poscache_docs as P
from oracle.oracle import OpLog as OracleOpLog

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import dt_amd  # noqa: E402
import poscache_model as M  # noqa: E402

# friendsforever under the shipped rule: every insert and delete round resolves one position
# (3,390 + 707), 2,252 of them from the cached block (1,855 inserts + 397 delete rounds)
FF_LOOKUPS, FF_SKIPS = 4097, 2252
CORNERS = ("skip_first", "skip_last", "miss_one_past", "skip_past_chunk", "skip_after_correction", "pass_drops",
           "pass_kept_nonzero", "pass_flips_after", "emptied_then_insert", "multi_round_deletes")


@pytest.fixture(scope="module")
def ff():
    o = dt_amd.ListOpLog.load_from(G.dt_bytes("friendsforever"))
    return o, M.model_oplog(o)


def test_friendsforever_text_and_blocks(ff):
    o, m = ff
    assert m.stats["text_len"] == 21362 and m.stats["blocks"] == 548 and m.stats["splits"] == 547
    assert M.text_of(o, m).decode() == G.trace("friendsforever_flat")["endContent"]


def test_friendsforever_counts_of_the_shipped_rule(ff):
    st = ff[1].stats
    assert st["disagree"] == 0
    assert (st["lookups"], st["skips"]) == (FF_LOOKUPS, FF_SKIPS)
    assert st["inserts"] + st["delete_rounds"] == FF_LOOKUPS
    assert st["same_block"] == 2414   # lookups whose answer is the cached block, prefix known or not
    assert (st["passes"], st["pass_drops"], st["pass_kept"]) == (2404, 1163, 1241)


def test_prefix_test_agrees_with_the_full_lookup_on_synthetic_merges():
    skips = 0
    for d in range(32):
        o = dt_amd.synth_merge_oplog(d, 5000)
        m = M.model_oplog(o)
        assert m.stats["disagree"] == 0, d
        skips += m.stats["skips"]
        if d < 4:
            assert M.text_of(o, m) == OracleOpLog.load_from(o.encode()).checkout_tip_bytes(), d
    assert skips > 0


def test_two_agent_document_reaches_the_corners():
    """The hand-built document of tests/test_gpu_poscache.py: more than 64 blocks, and every corner
    of the rule at least once (edits at the cached block's first and last visible item and one past
    it, a skipped lookup right after a pass corrected the prefix, passes that flip items before, in
    and after the cached block, a delete that empties the cached block followed by an insert at
    the same position, delete runs over several blocks)."""
    o = dt_amd.ListOpLog.load_from(P.two_agent_doc().encode())
    m = M.model_oplog(o)
    assert m.stats["disagree"] == 0 and m.stats["blocks"] > 64
    assert all(m.stats[k] > 0 for k in CORNERS), {k: m.stats[k] for k in CORNERS}
    assert M.text_of(o, m) == OracleOpLog.load_from(o.encode()).checkout_tip_bytes()
