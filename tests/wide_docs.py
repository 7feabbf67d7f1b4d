"""Fans: documents that sit exactly on the engine's 64-lane widths.  One agent ("base") types the
base text, then `width` agents each branch off the base tip and apply the same short shape of
edits, so the loaded document has a frontier `width` wide, `width` causal chains beside the base,
and, with the merge, an entry of `width` parents.  Built with the native ListOpLog (add_insert_at /
add_delete_at), deterministic, no checkout involved; the expected text of the single-op shapes is
kept by the plain models below, and tests/test_wide_docs.py checks them against the oracle.

A `.dt` file is written in walk order: every branch becomes one entry and the LVs are renumbered,
so tests read frontiers and versions off the loaded file.  as_parts() delivers the same kind of
document as a base part plus patches whose branches interleave, which keeps the LV order."""
import dt_amd

WIDTHS = (1, 2, 8, 9, 15, 16, 17, 32, 33, 63, 64, 65, 66, 96)
MIXED = ("ins_same2", "del_same2", "ins_own")
INS_AT, DEL_AT = 5, 2


def base_text(base_len=10):
    return "".join("0123456789"[k % 10] for k in range(base_len))


def agent_names(width):
    """Branch i's agent name: name order differs from agent-id order (37 is a unit mod 101: no
    two of up to 101 branches share a name)."""
    return ["w%03d" % ((i * 37 + 5) % 101) for i in range(width)]


def branch_char(i):
    """The 2-byte character branch i inserts in the one-character shape (distinct per branch)."""
    return chr(0x100 + i)


def _step(o, agent, parents, what, i):
    """One step of branch i's shape, in the branch's own coordinates.  (Shapes keep the deletes
    ahead of "ins_own", so the base characters 2 and 3 are still at positions 2 and 3.)"""
    if what == "ins_same":
        o.add_insert_at(agent, parents, INS_AT, branch_char(i))
    elif what == "ins_same2":
        o.add_insert_at(agent, parents, INS_AT, chr(65 + i % 26) + chr(97 + i % 26))
    elif what == "del_same":
        o.add_delete_at(agent, parents, DEL_AT, DEL_AT + 1)
    elif what == "del_same2":
        o.add_delete_at(agent, parents, DEL_AT, DEL_AT + 2)
    elif what == "ins_own":
        o.add_insert_at(agent, parents, i % 9, chr(0x3b1 + i % 24))
    else:
        raise ValueError(what)
    return len(o) - 1


def _start(width, base_len):
    assert base_len >= 10
    o = dt_amd.ListOpLog()
    base = o.get_or_create_agent_id("base")
    ids = [o.get_or_create_agent_id(n) for n in agent_names(width)]
    o.add_insert_at(base, [], 0, base_text(base_len))
    return o, base, ids


def fan(width, shape=MIXED, merge=False, base_len=10, interleave=False):
    """The oplog of a `width`-fan.  shape: a tuple of "ins_same" (one 2-byte character at position
    5), "ins_same2" (two ASCII characters there), "del_same" (base character 2), "del_same2" (base
    characters 2 and 3), "ins_own" (one character at position i % 9).  merge: "base" inserts "M"
    with every tip as a parent, the first branch agent types after the merge, and for width >= 2
    the second one inserts with the first width // 2 tips as parents.  interleave: the branches'
    steps round-robin in LV order (3 * width entries in memory; a file un-interleaves them)."""
    o, base, ids = _start(width, base_len)
    tips = [[base_len - 1] for _ in range(width)]
    order = ([(s, i) for s in range(len(shape)) for i in range(width)] if interleave
             else [(s, i) for i in range(width) for s in range(len(shape))])
    for s, i in order:
        tips[i] = [_step(o, ids[i], tips[i], shape[s], i)]
    flat = sorted(t[0] for t in tips)
    if merge:
        o.add_insert_at(base, flat, 0, "M")
        o.add_insert_at(ids[0], [len(o) - 1], 1, "t")
        if width >= 2:
            o.add_insert_at(ids[1], flat[:width // 2], 0, "h")
    return o


def merge_tail_chars(width):
    return 2 + (1 if width >= 2 else 0)


def as_parts(width, shape=MIXED, k=4, base_len=10):
    """(the oplog as built, the base as a `.dt` part, patches).  The patches add the branches k at
    a time, one patch per round of a group's steps, so the k branches of a group interleave
    round-robin in LV order: a peer that applies them in turn rebuilds the built oplog LV for LV."""
    o, base, ids = _start(width, base_len)
    part, f = o.encode(), o.local_frontier()
    patches = []
    for g in range(0, width, k):
        group = range(g, min(width, g + k))
        tips = {i: [base_len - 1] for i in group}
        for what in shape:
            for i in group:
                tips[i] = [_step(o, ids[i], tips[i], what, i)]
            patches.append(o.encode_from(f, dt_amd.ENCODE_PATCH))
            f = o.local_frontier()
    return o, part, patches


def _branch(o, agent, shape, i, base_len):
    tip = [base_len - 1]
    for what in shape:
        tip = [_step(o, agent, tip, what, i)]
    return tip[0]


def grown(width, extra, shape=MIXED, merge=False, base_len=10):
    """(the oplog as built, a `width`-fan as a `.dt` part, the patch after it): the patch adds
    `extra` further branches off the base tip and, with merge, fan()'s merge tail over all
    width + extra tips (extra = 0: the patch is the merge alone, its StartBranch version `width`
    wide)."""
    o, base, ids = _start(width + extra, base_len)
    tips = [_branch(o, ids[i], shape, i, base_len) for i in range(width)]
    part, f = o.encode(), o.local_frontier()
    tips += [_branch(o, ids[i], shape, i, base_len) for i in range(width, width + extra)]
    if merge:
        o.add_insert_at(base, sorted(tips), 0, "M")
        o.add_insert_at(ids[0], [len(o) - 1], 1, "t")
        if width + extra >= 2:
            o.add_insert_at(ids[1], sorted(tips)[:(width + extra) // 2], 0, "h")
    return o, part, o.encode_from(f, dt_amd.ENCODE_PATCH)


def halves(width, shape=MIXED, base_len=10):
    """(the oplog as built, part, patch): a fan whose `width` tips are one version `width` wide
    although no frontier on the way is: the part holds the first width // 2 branches and base's
    merge of them, the patch the other branches, children of the base tip like the first.  A peer
    that applies the two never holds a frontier past width - width // 2 + 1 (a file of the whole
    is written in walk order and may put every branch ahead of the merge).  The part is a file
    too: read the tips off the peer's oplog with branch_tips()."""
    o, base, ids = _start(width, base_len)
    tips = [_branch(o, ids[i], shape, i, base_len) for i in range(width // 2)]
    o.add_insert_at(base, sorted(tips), 0, "m")
    part, f = o.encode(), o.local_frontier()
    tips += [_branch(o, ids[i], shape, i, base_len) for i in range(width // 2, width)]
    return o, part, o.encode_from(f, dt_amd.ENCODE_PATCH)


def branch_tips(o, base_len=10):
    """The last LV of every branch of a fan whose branches are one entry each (as loaded from a
    file or applied from grown() / halves()): the entries whose only parent is the base tip, and
    the branch that shares the base's entry."""
    ents = o.export("entries")
    po, par = o.export("parent_offsets"), o.export("parents")
    tips = []
    for k, (_s, e) in enumerate(ents):
        if (k == 0 and e > base_len) or [int(p) for p in par[po[k]:po[k + 1]]] == [base_len - 1]:
            tips.append(int(e) - 1)
    return sorted(tips)


def widest_frontier(o):
    """The widest frontier while the entries are applied in order (what a decoder holds)."""
    ents = o.export("entries")
    po, par = o.export("parent_offsets"), o.export("parents")
    front, widest = set(), 0
    for k, (_s, e) in enumerate(ents):
        front -= {int(p) for p in par[po[k]:po[k + 1]]}
        front.add(int(e) - 1)
        widest = max(widest, len(front))
    return widest


# ---- plain models of the single-op shapes (they owe nothing to the oracle) -------------------------
def model_text(width, shape, base_len=10):
    """The text of an unmerged fan of a single-op shape.  Concurrent inserts at one position have
    the same origins and are ordered by agent name, ascending."""
    b = base_text(base_len)
    if shape == ("del_same",):
        return b[:DEL_AT] + b[DEL_AT + 1:]
    if shape == ("del_same2",):
        return b[:DEL_AT] + b[DEL_AT + 2:]
    if shape == ("ins_same",):
        names = agent_names(width)
        by_name = sorted(range(width), key=lambda i: names[i])
        return b[:INS_AT] + "".join(branch_char(i) for i in by_name) + b[INS_AT:]
    raise ValueError(shape)


def mixed_char_count(width, merge, base_len=10):
    return base_len - 2 + 3 * width + (merge_tail_chars(width) if merge else 0)


def toggle_passes(o):
    """[(entries, delete entries)] of every retreat / advance pass of the host plan."""
    cmds, tl = o.plan_commands(), o.plan_tlist()
    return [(n, sum((e >> 30) & 1 for e in tl[a:a + n])) for op, a, n, _ in cmds if (op & 15) == 2]
