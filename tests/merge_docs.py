"""Documents and helpers for the batched-merge tests (tests/test_merge_docs.py on the CPU,
tests/test_gpu_merge.py on the GPU).

small(): 15 LVs, three agents, six graph entries.  As (agent, parents, op):

    a []         ins 0 "abcdef"
    b [2]        ins 1 "XY"
    c [4]        ins 0 "Z"
    b [7]        del 0..2
    c [8]        del 1..2
    a [5,10,11]  ins 0 "M"
    a [12]       ins 1 "NO"

Between them its versions hold a `from` inside an entry whose suffix is merged, children hanging off
the consumed prefix and off the suffix of a partly consumed entry, a fast-forward prefix followed by
a walk, a two-LV `from`, a three-parent merge entry that waits for non-merges, and concurrent
deletes of one character.  A `.dt` file is written in walk order, so every LV a test uses is read
off the oplog loaded from small_bytes(), never off the oplog that wrote it."""
import itertools

import dt_amd

SMALL_TEXT = "MNOZYbcdef"


def small():
    o = dt_amd.ListOpLog()
    a, b, c = (o.get_or_create_agent_id(n) for n in ("a", "b", "c"))
    o.add_insert_at(a, [], 0, "abcdef")
    o.add_insert_at(b, [2], 1, "XY")
    o.add_insert_at(c, [4], 0, "Z")
    o.add_delete_at(b, [7], 0, 2)
    o.add_delete_at(c, [8], 1, 2)
    o.add_insert_at(a, [5, 10, 11], 0, "M")
    o.add_insert_at(a, [12], 1, "NO")
    return o


def small_bytes():
    return small().encode()


def versions(o):
    """ROOT, every single LV and every pair of concurrent LVs of oplog o."""
    n = len(o)
    out = [[]] + [[v] for v in range(n)]
    for x, y in itertools.combinations(range(n), 2):
        if o.dominators([x, y]) == [x, y]:
            out.append([x, y])
    return out


def all_pairs(o):
    vs = versions(o)
    return [(a, b) for a in vs for b in vs]


def exports(o):
    return o.export("ops").reshape(-1, 4), bytes(o.export("content")), o.export("char_offsets")


def per_char(oplog_exports, stream):
    """(lv, pos | None) stream -> [('I', pos, ch) | ('D', pos)] using an oplog's exported arrays."""
    ops, content, coff = oplog_exports
    kind = {}
    for lv, ln, _pos, kf in ops:
        for k in range(int(ln)):
            kind[int(lv) + k] = int(kf) & 1
    out = []
    for lv, x in stream:
        if x is None or x < 0:
            continue
        if kind[lv] == 0:
            b = int(coff[lv])
            out.append(("I", x, content[b:b + 4].decode("utf-8", errors="ignore")[:1]))
        else:
            out.append(("D", x))
    return out


def apply(text, ops):
    s = text
    for op in ops:
        s = s[:op[1]] + s[op[1] + 1:] if op[0] == "D" else s[:op[1]] + op[2] + s[op[1]:]
    return s


def oracle_records(ora, a, b):
    """The oracle's xf_operations_from as [(lv, pos | None)]."""
    return [(lv, None if x < 0 else x) for lv, x in ora.xf_operations_from(a, b)]
