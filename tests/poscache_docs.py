"""Documents for the replay's position cache (dt_replay.hip D.cpre / cpos; tools/poscache_model.py).

two_agent_doc(): two agents type about 6,700 characters (more than 64 blocks, so block positions
cross a chunk of the flat index) in epochs: from a common version each edits a region of its own --
one near the start, one far behind it, swapping sides every epoch -- and an insert that has both tips
as parents lands next to one branch's last edit.  Replaying one branch therefore retreats and
advances the other's items in blocks before or after the cached block, and a branch's own in the
block itself.  A branch's edits: typing, forward and backspace delete runs from 1 to 130 characters
(a run of 130 spans blocks), and the "held Delete key" -- delete the character at p, type one there,
delete that one again -- which walks through whole blocks one character at a time, so that a
delete leaves the cached block without a visible item and the next insert is at the same position.
The tests read off the model that these corners are reached."""
import random

import dt_amd

BASE_LEN = 4000
EPOCHS = 16


def _text(rng, n):
    return "".join(rng.choice("abcdefghijklmnopqrstuvwxyz ") for _ in range(n))


def _branch(o, rng, agent, tip, at, length, held):
    """One branch's edits around position `at` of a text `length` long (its own coordinates).
    Returns (tip, the position after its last edit, the text's length)."""
    def ins(p, s):
        nonlocal tip, length
        o.add_insert_at(agent, tip, p, s)
        tip = [len(o) - 1]
        length += len(s)

    def dele(p, n):
        nonlocal tip, length
        o.add_delete_at(agent, tip, p, p + n)
        tip = [len(o) - 1]
        length -= n

    p = at
    for _ in range(6):
        kind = rng.randrange(4)
        if kind == 0:      # typing
            s = _text(rng, rng.choice((1, 2, 5, 60, 120)))
            ins(p, s)
            p += len(s)
        elif kind == 1:    # a forward delete run
            n = rng.choice((1, 3, 40, 70, 130))
            dele(p, n)
        elif kind == 2:    # backspaces, one op each (the oplog joins them into a reversed run)
            for _ in range(rng.choice((1, 4, 30))):
                p -= 1
                dele(p, 1)
        else:              # somewhere else in the region
            p = at + rng.randrange(-150, 150)
    for _ in range(held):  # the held Delete key
        dele(p, 1)
        ins(p, "#")
        dele(p, 1)
    return tip, p, length


def two_agent_doc(seed=10):
    rng = random.Random(seed)
    o = dt_amd.ListOpLog()
    a, b = o.get_or_create_agent_id("alice"), o.get_or_create_agent_id("bob")
    o.add_insert_at(a, [], 0, _text(rng, BASE_LEN))
    tip = [len(o) - 1]
    length = BASE_LEN
    for e in range(EPOCHS):
        lo_agent, hi_agent = (a, b) if e % 2 == 0 else (b, a)
        lo_at, hi_at = 300 + 40 * e, length - 1200 + 40 * e
        near = (o, rng, lo_agent, tip, lo_at, length, 70 if e % 3 == 0 else 0)
        far = (o, rng, hi_agent, tip, hi_at, length, 70 if e % 3 == 1 else 0)
        if e % 4 < 2:   # the branch built second has the higher LVs
            (lo_tip, lo_p, lo_len), (hi_tip, hi_p, hi_len) = _branch(*near), _branch(*far)
        else:
            (hi_tip, hi_p, hi_len), (lo_tip, lo_p, lo_len) = _branch(*far), _branch(*near)
        d_lo = lo_len - length
        length = hi_len + d_lo
        # both tips as parents: next to the far branch's last edit (moved by the near branch's
        # net length), or next to the near branch's
        q = hi_p + d_lo if e % 4 < 2 else lo_p
        o.add_insert_at(a if e % 2 else b, sorted(lo_tip + hi_tip), q, _text(rng, 3))
        tip = [len(o) - 1]
        length += 3
    return o
