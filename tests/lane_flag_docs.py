"""Documents for the replay's lane flags (dt_replay.hip F_LIVE / F_VIS: a block held in registers
carries each item's liveness and visibility in the two top bits of its lane's word).

Every document opens with two agents typing concurrently from the empty version, so none is a linear
history (those never reach the tracker), and then edits from the merged version on.  Each is built
for a few corners of the flag handling; tests/test_lane_flag_docs.py reads off a host model of the
tracker (tools/poscache_model.py, instrumented there) that the corners are reached:

  fill_doc     one block filled to 62, then single characters at slot 0, at the last slot (63 + 1 =
               64: fits) and mid-block (64 + 1: splits); an insert at the end (origin_right END)
  runs_doc     runs of 1, 2, 63, 64, 65 and 130 at position 0, mid-text and at the end
  boundary_doc an insert whose origin_right is a deleted but live item; a forward delete of 130
               from inside a block, then the "held Delete key" (delete at p, type there, delete that)
               until a delete empties the cached block and the next insert lands at its position
  delete_doc   forward and backspace delete runs of 1, 64 and 130 that start inside a block
  tie_doc      three agents typing at one position from a common version (YjsMod, the tie broken by
               agent name), twice: at the end of the text and in front of a deleted item
  pass_doc     two branches from a common version, one typing 64 characters and one a single one at
               the same place: passes of exactly 64 entries and of 1, and the second branch's
               insert loads the block the pass just flipped (masks rebuilt from the counts)
"""
import random

import dt_amd

RUNS = (1, 2, 63, 64, 65, 130)
# The short documents end with a run of TAIL characters: every document then has more than eight
# blocks, which an LDS index sized for eight hands back to the HBM tier (that tier replays the
# document again from its first command, corners included).
TAIL = 600


def _text(rng, n):
    return "".join(rng.choice("abcdefghijklmnopqrstuvwxyz ") for _ in range(n))


class _Doc:
    """An oplog under construction: the current tip and the text's length at it."""

    def __init__(self, seed, names=("alice", "bob")):
        self.rng = random.Random(seed)
        self.o = dt_amd.ListOpLog()
        self.agents = [self.o.get_or_create_agent_id(n) for n in names]
        a, b = self.agents[:2]
        # the opening: both type five characters at position 0 of the empty text
        self.o.add_insert_at(a, [], 0, _text(self.rng, 5))
        ta = len(self.o) - 1
        self.o.add_insert_at(b, [], 0, _text(self.rng, 5))
        self.tip, self.length = [ta, len(self.o) - 1], 10

    def ins(self, pos, n, agent=0, tip=None):
        self.o.add_insert_at(self.agents[agent], self.tip if tip is None else tip, pos, _text(self.rng, n))
        if tip is None:
            self.tip, self.length = [len(self.o) - 1], self.length + n
        return [len(self.o) - 1]

    def dele(self, pos, n, agent=0):
        self.o.add_delete_at(self.agents[agent], self.tip, pos, pos + n)
        self.tip, self.length = [len(self.o) - 1], self.length - n

    def backspace(self, pos, n, agent=0):
        """n single deletes, each of the character before the cursor (joined into a reversed run)."""
        for _ in range(n):
            pos -= 1
            self.dele(pos, 1, agent)
        return pos

    def join(self, tips, added):
        self.tip, self.length = sorted(t for tip in tips for t in tip), self.length + added


def fill_doc():
    d = _Doc(1)
    d.ins(10, 52)           # the first block: 62 items
    d.ins(0, 1)             # slot 0 -> 63
    d.ins(63, 1)            # the last slot, at the text's end: 63 + 1 = 64, fits
    d.ins(30, 1)            # mid-block, 64 + 1: splits
    d.ins(d.length, 3)      # the end again, now in the second block
    d.ins(15, 1)            # mid-block, and it fits
    d.ins(d.length, TAIL)
    return d.o


def runs_doc():
    d = _Doc(2)
    for k in RUNS:
        d.ins(0, k)
        d.ins(d.length // 2, k)
        d.ins(d.length, k)
        d.ins(7, 1)         # keeps the next run at position 0 a run of its own
    return d.o


def boundary_doc():
    d = _Doc(3)
    d.dele(4, 1)
    d.ins(4, 2)             # origin_right: the character just deleted (live, not visible)
    d.ins(d.length, 300)
    d.dele(40, 130)         # from inside a block over whole blocks
    d.ins(3, 1)             # (keeps the next delete a run of its own)
    p = 41
    for _ in range(80):     # the held Delete key
        d.dele(p, 1)
        d.ins(p, 1)
        d.dele(p, 1)
    d.ins(p, 2)
    return d.o


def delete_doc():
    d = _Doc(4)
    d.ins(10, 700)
    for n in (1, 64, 130):
        d.dele(40, n)                       # forward, from inside a block
        d.ins(3, 1)
        d.backspace(d.length - 20, n)       # backspaces, from inside a later block
        d.ins(5, 1)
    return d.o


def tie_doc():
    d = _Doc(5, ("alice", "bob", "carol"))
    for where in ("end", "before_deleted"):
        if where == "before_deleted":
            d.dele(6, 2)
        pos = d.length if where == "end" else 6
        base = d.tip
        tips = [d.ins(pos, n, agent=g, tip=base) for g, n in ((2, 3), (0, 1), (1, 2))]
        d.join(tips, 6)
        d.ins(2, 1)
    d.ins(d.length, TAIL)
    return d.o


def pass_doc():
    d = _Doc(6)
    d.ins(10, 40)
    for at, first in ((20, 64), (d.length, 1)):   # the branch with the lower LVs is retreated
        base = d.tip
        one = d.ins(at, first, agent=0, tip=base)
        other = d.ins(at, 65 - first, agent=1, tip=base)
        d.join([one, other], 65)
        d.ins(1, 1)
    d.ins(d.length, TAIL)
    return d.o


BUILDERS = dict(fill=fill_doc, runs=runs_doc, boundary=boundary_doc, delete=delete_doc, tie=tie_doc, passes=pass_doc)


def all_docs():
    """{name: oplog}, in a fixed order."""
    return {name: f() for name, f in BUILDERS.items()}
