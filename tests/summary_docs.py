"""Documents and summaries shared by test_summary_api.py (host) and test_gpu_summary.py (device):
the reference's own vectors from src/causalgraph/summary.rs (`summary_smoke`, `intersect_summary`),
documents whose agent runs are not in seq order, and random summaries."""
import random

import dt_amd

# the summary both reference tests intersect with (summary.rs:414-423)
REF_VS = [("seph", [(0, 10)]), ("mike", [(0, 5)])]


def smoke_doc():
    """summary_smoke (summary.rs:297-373): seph 0..5 at ROOT, mike 0..5 at ROOT, seph 5..10 after
    [4], then, after a gap, mike 15..20 after [4, 9].  Returns (oplog before the gap, oplog with
    it).  The public API assigns seqs densely, so mike's 5..15 are added on a side branch and left
    out by taking the history of the rest."""
    o = dt_amd.ListOpLog()
    seph, mike = o.get_or_create_agent_id("seph"), o.get_or_create_agent_id("mike")
    o.add_insert_at(seph, [], 0, "a" * 5)          # LVs 0..4
    o.add_insert_at(mike, [], 0, "b" * 5)          # 5..9
    o.add_insert_at(seph, [4], 0, "c" * 5)         # 10..14
    before = o.history([9, 14])
    o.add_insert_at(mike, [9], 0, "x" * 10)        # 15..24: mike 5..15, not to be kept
    o.add_insert_at(mike, [4, 9], 0, "d" * 5)      # 25..29: mike 15..20
    return before, o.history([14, 29])


def sparse_doc():
    """intersect_summary's oplog (summary.rs:438-446): seph 1..5 -> LVs 0..3 and seph 8..9 -> LV 4,
    both at ROOT, and an agent mike without ops.  One agent commits on concurrent branches
    (add_insert_at with explicit parents); the host encoder writes the patch that leaves the other
    branches out, but an empty oplog refuses it (its StartBranch names the left-out ops:
    BaseVersionUnknown), so the kept branches go through history(), encode() and decode_and_add()
    into an oplog that already knows both names."""
    o = dt_amd.ListOpLog()
    seph = o.get_or_create_agent_id("seph")
    o.add_insert_at(seph, [], 0, "a")              # seph 0      LV 0
    o.add_insert_at(seph, [], 0, "bcde")           # seph 1..5   LVs 1..4
    o.add_insert_at(seph, [0], 1, "fgh")           # seph 5..8   LVs 5..7
    o.add_insert_at(seph, [], 0, "i")              # seph 8..9   LV 8
    kept = o.history([4, 8])
    out = dt_amd.ListOpLog()
    out.get_or_create_agent_id("seph")
    out.get_or_create_agent_id("mike")
    out.decode_and_add(kept.encode())
    assert [list(map(int, r)) for r in out.export("agent_runs")] == [[0, 4, 0, 1], [4, 1, 0, 8]]
    return out


def sparse_doc_with_kaarina():
    """... then kaarina 0..10 after [3, 4] (summary.rs:474-478); returns (oplog, v = its last LV)."""
    o = sparse_doc()
    k = o.get_or_create_agent_id("kaarina")
    return o, o.add_insert_at(k, [3, 4], 0, "0123456789")


def reordered_parts(sparse=False):
    """One agent's runs where LV order != seq order: x types two concurrent spans (three with
    `sparse`), and a peer receives the later span first.  Returns (part, patch): a `.dt` file with the
    later span and a second one with the first span, to be merged in that order.  With `sparse` the
    middle span x 5..10 never arrives, so a gap lies between the re-ordered pieces."""
    o = dt_amd.ListOpLog()
    x, y = o.get_or_create_agent_id("x"), o.get_or_create_agent_id("y")
    o.add_insert_at(x, [], 0, "aaaaa")             # x 0..5    LVs 0..4
    o.add_insert_at(x, [], 0, "bbbbb")             # x 5..10   LVs 5..9
    last = 9
    if sparse:
        o.add_insert_at(x, [], 0, "ccccc")         # x 10..15  LVs 10..14
        last = 14
    o.add_insert_at(y, [last], 0, "yy")            # y 0..2 on top of the later span
    return o.history([last + 2]).encode(), o.history([4]).encode()


def reordered_host(sparse=False):
    part, patch = reordered_parts(sparse)
    o = dt_amd.ListOpLog.load_from(part)
    o.decode_and_add(patch)
    runs = [list(map(int, r)) for r in o.export("agent_runs")]
    assert runs == ([[0, 5, 0, 10], [5, 2, 1, 0], [7, 5, 0, 0]] if sparse else [[0, 5, 0, 5], [5, 2, 1, 0], [7, 5, 0, 0]])
    return o


def alternating_doc(rounds=70, run_len=2):
    """2 * rounds agent runs of two alternating agents, run_len seqs each: 140 runs (the sweep goes
    64 runs a step), 70 known pieces in one range."""
    o = dt_amd.ListOpLog()
    a, b = o.get_or_create_agent_id("ann"), o.get_or_create_agent_id("bob")
    for _ in range(rounds):
        o.add_insert(a, 0, "a" * run_len)
        o.add_insert(b, 0, "b" * run_len)
    assert len(o.export("agent_runs")) == 2 * rounds
    return o


def many_agents_doc(n=70):
    """n agents (wide_docs' scrambled names: name order is not id order) typing in turn, two seqs
    each, then once more in reverse: more agents than the 64 a resolve step compares."""
    import wide_docs
    o = dt_amd.ListOpLog()
    ids = [o.get_or_create_agent_id(name) for name in wide_docs.agent_names(n)]
    for a in ids + ids[::-1]:
        o.add_insert(a, 0, "ab")
    return o


def random_summary(rng, o, n_entries=None):
    """A random summary for oplog o: known names, unknown ones, names that are prefixes of one
    another, duplicates; ranges that clip a run at its first, middle and last seq, reach past the
    agent's seqs, end at 2^40, overlap one another."""
    names = [bytes(n).decode() for n in o.export("agent_names")]
    runs = [tuple(int(x) for x in r) for r in o.export("agent_runs")]
    pool = names + ["nobody", "ROOT", "", "z" * 60] + [n[:-1] for n in names if len(n) > 1] + [n + "0" for n in names[:3]]
    out = []
    for _ in range(rng.randrange(0, 7) if n_entries is None else n_entries):
        name = rng.choice(pool)
        rs = []
        for _ in range(rng.randrange(0, 5)):
            mine = [(seq, seq + ln) for _lv, ln, a, seq in runs if a < len(names) and names[a] == name]
            how = rng.randrange(6)
            if mine and how < 4:
                s0, e0 = rng.choice(mine)
                s1, e1 = rng.choice(mine)
                lo = min(s0, s1) + rng.choice((0, 0, 1, (e0 - s0) // 2))
                hi = max(e0, e1) - rng.choice((0, 0, 1, (e1 - s1) // 2))
                if how == 3:
                    lo, hi = s0, s0 + 1     # exactly a run's first seq
                if how == 2:
                    lo, hi = e0 - 1, e0     # exactly its last
                if lo >= hi:
                    hi = lo + 1
                rs.append((lo, hi))
            elif how == 4:
                lo = rng.randrange(0, 50)
                rs.append((lo, 1 << 40))
            else:
                lo = rng.randrange(0, 400)
                rs.append((lo, lo + rng.randrange(1, 200)))
        out.append((name, rs))
    if out and rng.randrange(3) == 0:
        out.append(rng.choice(out))   # a duplicate entry
    return out


def random_frontier(rng, o):
    return [rng.randrange(len(o)) for _ in range(rng.randrange(0, 4))] if len(o) else []
