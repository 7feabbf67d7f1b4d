"""The blame model and the documents of the blame tests (tests/test_blame_docs.py on the CPU,
tests/test_gpu_blame.py on the GPU).

The model is the CPU oracle's, never the device's: OracleOpLog.xf_operations() (at a version,
xf_operations_from([], version)) applied in order to a Python list of LVs -- an insert LV with
xf >= 0 does list.insert(xf, lv), a delete del list[xf], -1 nothing -- gives the text as LVs in
document order; decoded()["agent_runs"] (lv_start, len, agent, seq_start) maps each LV to
(agent name, seq); maximal runs follow by grouping.  A `.dt` file is written in walk order, so
every builder returns encoded bytes and both sides load those: the LVs are then the same."""
import bisect

import dt_amd
from oracle.oracle import OpLog as OracleOpLog


def model_lvs(ora, version=None):
    """The text of `ora` (at the tip, or at `version`) as the list of its characters' LVs."""
    dec = ora.decoded()
    kind = [k for k, _pos, _cb in dec["lv"]]
    stream = ora.xf_operations() if version is None else ora.xf_operations_from([], list(version))
    out = []
    for lv, xf in stream:
        if xf < 0:
            continue
        if kind[lv] == 0:
            out.insert(xf, lv)
        else:
            del out[xf]
    return out


def lv_text(ora, lvs) -> bytes:
    """The characters of the LVs, joined."""
    dec = ora.decoded()
    content = dec["content"]
    out = bytearray()
    for lv in lvs:
        cb = dec["lv"][lv][2]
        b0 = content[cb]
        n = 1 if b0 < 0x80 else 2 if (b0 & 0xE0) == 0xC0 else 3 if (b0 & 0xF0) == 0xE0 else 4
        out += content[cb:cb + n]
    return bytes(out)


def lv_runs(lvs):
    """[(lv, len)]: maximal runs of consecutive LVs, not yet split by agent."""
    out = []
    for lv in lvs:
        if out and out[-1][0] + out[-1][1] == lv:
            out[-1][1] += 1
        else:
            out.append([lv, 1])
    return [tuple(r) for r in out]


def model_runs(ora, version=None):
    """[(lv, len, agent name, seq)]: the blame's maximal runs in text order."""
    dec = ora.decoded()
    aruns = dec["agent_runs"]
    starts = [r[0] for r in aruns]
    names = dec["agent_names"]
    out = []
    for lv in model_lvs(ora, version):
        s, _n, agent, seq0 = aruns[bisect.bisect_right(starts, lv) - 1]
        name, seq = names[agent], seq0 + (lv - s)
        if out and out[-1][0] + out[-1][1] == lv and out[-1][2] == name and out[-1][3] + out[-1][1] == seq:
            out[-1][1] += 1
        else:
            out.append([lv, 1, name, seq])
    return [tuple(r) for r in out]


def spans_of(runs):
    """Model runs as Batch.blame_spans gives them: (agent name bytes, seq_start, seq_end, char_start,
    char_end), adjacent runs of one agent with continuing seqs joined whatever their LVs -- the form
    that does not depend on an oplog's LV numbering."""
    out, at = [], 0
    for _lv, n, name, seq in runs:
        if out and out[-1][0] == name.encode() and out[-1][2] == seq:
            out[-1] = out[-1][:2] + (seq + n, out[-1][3], at + n)
        else:
            out.append((name.encode(), seq, seq + n, at, at + n))
        at += n
    return out


# ---- builders: every one returns encoded `.dt` bytes ---------------------------------------------
WIDTHS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]


def _new(*names):
    o = dt_amd.ListOpLog()
    return (o,) + tuple(o.get_or_create_agent_id(n) for n in names)


def one_run(n):
    """One author types n characters as one run."""
    o, a = _new("solo")
    o.add_insert(a, 0, "".join(chr(ord("a") + k % 26) for k in range(n)))
    return o.encode()


def alternating(n):
    """Two agents alternate character by character through the graph: each op's parent is the
    other's last, so the history is a chain of n one-LV agent runs."""
    o, a, b = _new("ann", "bob")
    last = []
    for k in range(n):
        lv = o.add_insert_at(a if k % 2 == 0 else b, last, k, chr(ord("a") + k % 26))
        last = [lv]
    return o.encode()


def deleted_middle():
    o, a = _new("solo")
    o.add_insert(a, 0, "abcde")
    o.add_delete_without_content(a, 2, 3)
    return o.encode()


def insert_in_middle():
    o, a = _new("solo")
    o.add_insert(a, 0, "abcde")
    o.add_insert(a, 2, "XY")
    return o.encode()


def insert_deleted_again():
    """The insert into the middle is deleted again: LVs 0-1 and 2-4 are adjacent once more and must
    come back as one run."""
    o, a = _new("solo")
    o.add_insert(a, 0, "abcde")
    o.add_insert(a, 2, "XY")
    o.add_delete_without_content(a, 2, 4)
    return o.encode()


def backspaces():
    o, a = _new("solo")
    o.add_insert(a, 0, "abcdefghij")
    for p in (8, 7, 6, 5):   # a backspace run: single deletes at decreasing positions
        o.add_delete_without_content(a, p - 1, p)
    o.add_insert(a, 4, "Z")
    return o.encode()


def all_deleted():
    o, a = _new("solo")
    o.add_insert(a, 0, "abcdef")
    o.add_delete_without_content(a, 0, 6)
    return o.encode()


def all_deleted_concurrently():
    """Two agents delete the same text concurrently: a document with history and no text, on the
    tracker."""
    o, a, b = _new("ann", "bob")
    t = o.add_insert_at(a, [], 0, "aaa")
    o.add_delete_at(a, [t], 1, 2)
    o.add_delete_at(b, [t], 0, 3)
    return o.encode()


def no_inserts():
    """A document with no inserts: an empty oplog."""
    return dt_amd.ListOpLog().encode()


def agent_boundary():
    """A types x (lv 0), B with parent lv 0 types y after it (lv 1): consecutive LVs, adjacent in the
    text, two runs."""
    o, a, b = _new("A", "B")
    x = o.add_insert_at(a, [], 0, "x")
    o.add_insert_at(b, [x], 1, "y")
    return o.encode()


def tie_break():
    """The three-agent concurrent insert of tests/test_gpu_parity.py: "cccaaabbb"."""
    o, a, b = _new("a", "b")
    o.add_insert_at(a, [], 0, "aaa")
    o.add_insert_at(b, [], 0, "bbb")
    o.add_insert_at(a, [2, 5], 0, "ccc")
    return o.encode()


def utf8():
    """2-, 3- and 4-byte characters, typed by two agents, some deleted."""
    o, a, b = _new("ann", "bob")
    x = o.add_insert_at(a, [], 0, "hé€😀llo")
    y = o.add_insert_at(b, [x], 3, "ß中🎉")
    z = o.add_delete_at(a, [y], 1, 2)
    o.add_insert_at(b, [x], 0, "文é")
    del z
    return o.encode()


def two_blocks(n):
    """Two agents each type n characters at position 0 concurrently: 2n inserted characters in two
    op runs (the size picks the replay tier), two runs."""
    o, a, b = _new("ann", "bob")
    o.add_insert_at(a, [], 0, "x" * n)
    o.add_insert_at(b, [], 0, "y" * n)
    return o.encode()


def linear_turns():
    """A linear history (one graph entry) typed by two agents in turns of 1, 2 and 70 characters,
    with edits that split pieces: pieces split at agent-run boundaries, and the first piece spans
    more than two agent runs."""
    o, a, b = _new("ann", "bob")
    at = 0
    for k, n in enumerate([1, 2, 70, 1, 2, 70, 2, 1]):
        o.add_insert(a if k % 2 == 0 else b, at, "".join(chr(ord("a") + (at + j) % 26) for j in range(n)))
        at += n
    o.add_delete_without_content(b, 40, 80)    # inside the 70-character turns
    o.add_insert(a, 10, "QRS")                 # splits a piece inside a turn
    o.add_delete_without_content(a, 105, 106)  # one character of the last long turn
    return o.encode()


def linear_long(n_runs=200):
    """A linear document of more than 63 op runs by two agents, so several fast-forward segments
    compose: inserts at scattered positions, deletes between them."""
    import random
    rng = random.Random(7)
    o, a, b = _new("ann", "bob")
    n = 0
    for k in range(n_runs):
        who = a if (k // 3) % 2 == 0 else b
        if k % 3 == 2 and n > 4:
            p = rng.randrange(n - 2)
            o.add_delete_without_content(who, p, p + 2)
            n -= 2
        else:
            s = "".join(rng.choice("abcdefgh") for _ in range(rng.randint(1, 6)))
            p = rng.randint(0, n)
            o.add_insert(who, p, s)
            n += len(s)
    return o.encode()


def small_docs():
    """name -> `.dt` bytes of every small hand-built document."""
    docs = {"deleted_middle": deleted_middle(), "insert_in_middle": insert_in_middle(),
            "insert_deleted_again": insert_deleted_again(), "backspaces": backspaces(),
            "all_deleted": all_deleted(), "no_inserts": no_inserts(), "all_deleted_concurrently": all_deleted_concurrently(),
            "agent_boundary": agent_boundary(), "tie_break": tie_break(), "utf8": utf8(),
            "linear_turns": linear_turns(), "linear_long": linear_long()}
    for n in WIDTHS:
        docs[f"one_run_{n}"] = one_run(n)
        docs[f"alternating_{n}"] = alternating(n)
    return docs
