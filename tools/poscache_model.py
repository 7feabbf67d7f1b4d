"""CPU model of the flat-tier replay's position cache (dt_replay.hip: D.cb / cpre / cpos).

Replays a document's host plan (plan_commands() / plan_tlist()) through a sequential model of
the tracker -- 64-slot blocks cut at the insert point clamped to [16, 48], the one-block register
cache dropped when a retreat/advance pass flips an item in the cached block -- and applies the
cached-prefix rule the kernel ships:

  cpre  visible items before the cached block cb (None: unknown), cpos its position in ord[]
  an insert at pos > 0 skips the index scan iff pos - 1 - cpre < visible(cb) (unsigned),
  a delete round at pos iff pos - cpre < visible(cb)
  after an insert: cpre is kept iff the run ended in the block the lookup returned
  after a delete round: cpre = pos - rank
  a pass (in the kernel's 64-entry chunks) that leaves cb cached adds the visibility flips in
  blocks before cb to cpre

Every skipped lookup is checked against the full scan.  The lookup / skip counts are what the
instrumented kernel reports (DTGPU_DEBUG=2: doc_stats n_lookup / n_lookup_skip) for a document
replayed whole.

Usage: python tools/poscache_model.py friendsforever [synth:SEED ...]
"""
import bisect
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BLK = 64
ROOT_ID = 0xFFFFFFFF
END_ID = 0xFFFFFFFE
CMD_INS, CMD_DEL, CMD_TOG = 0, 1, 2


class ModelError(Exception):
    pass


def cut_point(s):
    return min(max(s, 16), 48)


class Model:
    def __init__(self, cmds, tlist, aruns, n_lv):
        self.cmds, self.tlist, self.n_lv = cmds, tlist, n_lv
        self.arun_lv = aruns[0::4]
        self.arun_rank = aruns[1::4]
        self.arun_seq = aruns[2::4]
        self.cnt = [0] * n_lv        # 0 not inserted yet, 1 visible, k >= 2 deleted k - 1 times
        self.blk = [0] * n_lv
        self.ol = [0] * n_lv         # Ins: origin_left; Del: the item it deleted
        self.orr = [0] * n_lv
        self.items = [[]]            # per block, document order
        self.bvis = [0]              # per block: visible items
        self.blive = [0]             # per block: live items
        self.dirty = [False]         # per block: a pass changed counts since its masks were built
        self.ord = [0]               # block by position
        self.opos = [0]              # position by block
        self.cb = None               # the block cached in registers
        self.cpre = None
        self.cpos = 0
        self.stats = dict(lookups=0, skips=0, same_block=0, disagree=0, splits=0, loads=0, dirty_loads=0,
                          inserts=0, delete_rounds=0, passes=0, pass_drops=0, pass_kept=0, pass_kept_nonzero=0,
                          flips_before=0,
                          # which corners of the rule a document reaches (tests assert their inputs do)
                          skip_first=0, skip_last=0, miss_one_past=0, skip_past_chunk=0, skip_after_correction=0,
                          pass_flips_after=0, emptied_then_insert=0, multi_round_deletes=0)
        self._corrected = False      # the last pass changed cpre and no lookup has used it yet
        self._emptied_at = None      # the last delete round emptied the cached block at this position

    # ---- queries
    def find_vis(self, p):
        base = 0
        for q, b in enumerate(self.ord):
            v = self.bvis[b]
            if base + v > p:
                return b, p - base, base, q
            base += v
        raise ModelError(f"find_vis({p}) past the end")

    def lookup(self, p):
        """Block and rank of visible item p: from the cached block when the prefix test says so."""
        st = self.stats
        st["lookups"] += 1
        full = self.find_vis(p)
        if self.cb is not None and full[0] == self.cb:
            st["same_block"] += 1
        if self.cb is not None and self.cpre is not None and p - self.cpre == self.bvis[self.cb]:
            st["miss_one_past"] += 1
        corrected, self._corrected = self._corrected, False
        if self.cb is not None and self.cpre is not None and 0 <= p - self.cpre < self.bvis[self.cb]:
            st["skips"] += 1
            st["skip_first"] += p == self.cpre
            st["skip_last"] += p - self.cpre == self.bvis[self.cb] - 1
            st["skip_past_chunk"] += self.cpos >= 64
            st["skip_after_correction"] += corrected
            got = (self.cb, p - self.cpre, self.cpre, self.cpos)
            if got != full:
                st["disagree"] += 1
            return full   # (a disagreement is counted, never followed)
        return full

    def slot_of_rank(self, b, k):
        for s, it in enumerate(self.items[b]):
            if self.cnt[it] == 1:
                if k == 0:
                    return s
                k -= 1
        raise ModelError("rank past the block's visible items")

    def load(self, b):
        self.stats["loads"] += 1
        if self.dirty[b]:
            self.stats["dirty_loads"] += 1
            self.dirty[b] = False

    def key(self, item):
        b = self.blk[item]
        return (self.opos[b] << 6) | self.items[b].index(item)

    def agent_of(self, lv):
        j = bisect.bisect_right(self.arun_lv, lv) - 1
        return self.arun_rank[j], self.arun_seq[j] + (lv - self.arun_lv[j])

    def next_live_block(self, b):
        for q in range(self.opos[b] + 1, len(self.ord)):
            if self.blive[self.ord[q]]:
                return self.ord[q]
        return None

    # ---- maintenance
    def split_block(self, b, cut):
        self.stats["splits"] += 1
        b2 = len(self.items)
        moved = self.items[b][cut:]
        del self.items[b][cut:]
        self.items.append(moved)
        for it in moved:
            self.blk[it] = b2
        v2 = sum(1 for it in moved if self.cnt[it] == 1)
        l2 = sum(1 for it in moved if self.cnt[it] != 0)
        self.bvis.append(v2)
        self.blive.append(l2)
        self.bvis[b] -= v2
        self.blive[b] -= l2
        self.dirty.append(False)
        p = self.opos[b] + 1
        self.ord.insert(p, b2)
        self.opos.append(p)
        for q in range(p, len(self.ord)):
            self.opos[self.ord[q]] = q
        return b2

    def insert_run(self, b, s, lv, k, ol, orr):
        for j in range(k):
            it = lv + j
            self.cnt[it] = 1
            self.ol[it] = ol if j == 0 else it - 1
            self.orr[it] = orr
        while k > 0:
            row = self.items[b]
            if len(row) == BLK:
                cut = cut_point(s)
                b2 = self.split_block(b, cut)
                if s > cut:
                    b, s = b2, s - cut
                continue
            m = min(k, BLK - len(row))
            row[s:s] = range(lv, lv + m)
            for it in range(lv, lv + m):
                self.blk[it] = b
            self.bvis[b] += m
            self.blive[b] += m
            lv += m
            k -= m
            s += m
        self.cb = b

    # ---- commands
    def do_insert(self, lv, k, pos):
        self.stats["inserts"] += 1
        self.stats["emptied_then_insert"] += self._emptied_at == pos
        self._emptied_at = None
        if pos == 0:   # counted as a lookup (every edit resolves one position), never as a skip
            self.stats["lookups"] += 1
            b, kk, pre, bpos = self.ord[0], 0, 0, 0
        else:
            b, kk, pre, bpos = self.lookup(pos - 1)
        b_found = b
        if b != self.cb:
            self.load(b)
        s, ol = 0, ROOT_ID
        if pos:
            s0 = self.slot_of_rank(b, kk)
            ol = self.items[b][s0]
            s = s0 + 1
        row = self.items[b]
        rs = next((i for i in range(s, len(row)) if self.cnt[row[i]] != 0), None)
        if rs is not None:
            rb, orr = b, row[rs]
            direct = rs == s
        else:
            rb = self.next_live_block(b)
            if rb is not None:
                self.load(rb)
                rrow = self.items[rb]
                rs = next(i for i in range(len(rrow)) if self.cnt[rrow[i]] != 0)
                orr = rrow[rs]
            else:
                rs, orr = 0, END_ID
            if s < len(row):
                direct = False
            else:
                q = self.opos[b] + 1
                nx = self.ord[q] if q < len(self.ord) else None
                direct = nx is None or (rb == nx and rs == 0)
        if not direct:
            b0 = b
            b, s = self.yjs_scan(b, s, rb, rs, ol, orr, lv)
            if b != b0 and b != self.cb:
                self.load(b)
        self.cb = None
        self.insert_run(b, s, lv, k, ol, orr)
        if self.cb == b_found:
            self.cpre, self.cpos = pre, bpos
        else:
            self.cpre = None

    def yjs_scan(self, b, s, rb, rs, ol_new, orr_new, lv):
        """YjsMod integrate over the not-inserted-yet items between the cursor and origin_right,
        one candidate at a time (the kernel resolves a block of candidates with ballots)."""
        my_l = 0 if ol_new == ROOT_ID else self.key(ol_new) + 1
        my_r = 1 << 62 if orr_new == END_ID else self.key(orr_new)
        new_agent = self.agent_of(lv)
        scanning, scan = False, (b, s)
        cb, cs = b, s
        while True:
            if cs >= len(self.items[cb]):
                q = self.opos[cb] + 1
                if q >= len(self.ord):
                    break
                cb, cs = self.ord[q], 0
                continue
            if cb == rb and cs >= rs:
                break
            o = self.items[cb][cs]
            kl = 0 if self.ol[o] == ROOT_ID else self.key(self.ol[o]) + 1
            if kl < my_l:
                break
            if kl == my_l:
                if self.orr[o] == orr_new:
                    if new_agent < self.agent_of(o):
                        break
                    scanning = False
                else:
                    kr = 1 << 62 if self.orr[o] == END_ID else self.key(self.orr[o])
                    if kr < my_r:
                        if not scanning:
                            scanning, scan = True, (cb, cs)
                    else:
                        scanning = False
            cs += 1
        return scan if scanning else (cb, cs)

    def do_delete(self, lv, n, pos, fwd):
        j0 = 0
        self._emptied_at = None
        while j0 < n:
            self.stats["delete_rounds"] += 1
            b, kk, _pre, bpos = self.lookup(pos)
            if b != self.cb:
                self.load(b)
            take = min(self.bvis[b] - kk, n - j0)
            if take <= 0:
                raise ModelError("delete round without a visible item")
            r = 0
            for it in self.items[b]:
                if self.cnt[it] == 1:
                    if kk <= r < kk + take:
                        j = j0 + (r - kk)
                        dlv = lv + j if fwd else lv + n - 1 - j
                        self.cnt[it] = 2
                        self.ol[dlv] = it
                    r += 1
            self.bvis[b] -= take
            self.cb, self.cpre, self.cpos = b, pos - kk, bpos
            self.stats["multi_round_deletes"] += j0 > 0 and j0 + take >= n
            j0 += take
        self._emptied_at = pos if self.bvis[self.cb] == 0 else None

    def toggle(self, off, n):
        st = self.stats
        st["passes"] += 1
        had_cache = self.cb is not None
        corr = after = 0
        self._emptied_at = None
        for c0 in range(off, off + n, 64):   # the kernel's 64-entry chunks; lanes sharing an item merged
            delta, neg = {}, {}
            for e in self.tlist[c0:min(c0 + 64, off + n)]:
                lv = e & 0x3FFFFFFF
                item = self.ol[lv] if (e >> 30) & 1 else lv
                adv = e >> 31
                delta[item] = delta.get(item, 0) + (1 if adv else -1)
                neg[item] = neg.get(item, 0) + (0 if adv else -1)
            flips = []
            for item, d in delta.items():
                oc = self.cnt[item]
                nc = oc + d
                if oc + neg[item] < 0:
                    raise ModelError("retreat below zero")
                self.cnt[item] = nc
                fv, fl = (oc == 1) != (nc == 1), (oc != 0) != (nc != 0)
                if fv or fl:
                    flips.append((self.blk[item], (1 if nc == 1 else -1) if fv else 0,
                                  (1 if nc != 0 else -1) if fl else 0))
            if any(b == self.cb for b, _dv, _dl in flips):
                self.cb = self.cpre = None
            for b, dv, dl in flips:
                self.bvis[b] += dv
                self.blive[b] += dl
                self.dirty[b] = True
                if self.cpre is not None and dv and self.opos[b] < self.cpos:
                    self.cpre += dv
                    corr += 1
                elif self.cpre is not None and dv:
                    after += 1
        if had_cache:
            if self.cb is None:
                st["pass_drops"] += 1
            else:
                st["pass_kept"] += 1
                if corr and self.cpre is not None:
                    st["pass_kept_nonzero"] += 1
                    st["flips_before"] += corr
                    self._corrected = True
                if after and self.cpre is not None:
                    st["pass_flips_after"] += 1

    def run(self):
        for op, a, n, pos in self.cmds:
            code = op & 15
            if code == CMD_INS:
                self.do_insert(a, n, pos)
            elif code == CMD_DEL:
                self.do_delete(a, n, pos, bool(op & 16))
            elif code == CMD_TOG:
                self.toggle(a, n)
            else:
                raise ModelError(f"unknown command {op}")
        st = self.stats
        st["blocks"] = len(self.items)
        st["text_len"] = sum(self.bvis)
        return st

    def visible_items(self):
        return [it for b in self.ord for it in self.items[b] if self.cnt[it] == 1]


def model_oplog(oplog):
    """Run the model on a dt_amd.ListOpLog's host plan; returns the Model (stats in .stats)."""
    m = Model(oplog.plan_commands(), oplog.plan_tlist(), oplog.agent_runs(), len(oplog))
    m.run()
    return m


def text_of(oplog, m):
    """The model's final text, from the oplog's inserted content."""
    content, cbyte = oplog.ins_content(), oplog.char_offsets()
    out = bytearray()
    for it in m.visible_items():
        o = cbyte[it]
        c = content[o]
        out += content[o:o + (1 if c < 0x80 else 2 if (c & 0xE0) == 0xC0 else 3 if (c & 0xF0) == 0xE0 else 4)]
    return bytes(out)


def main():
    sys.path.insert(0, os.path.join(ROOT, "diamond-types_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dt_amd
    import golden_data as G
    for name in sys.argv[1:] or ["friendsforever"]:
        if name.startswith("synth:"):
            o = dt_amd.synth_merge_oplog(int(name.split(":")[1]), 5000)
        else:
            o = dt_amd.ListOpLog.load_from(G.dt_bytes(name))
        st = model_oplog(o).stats
        print(name, " ".join(f"{k}={v}" for k, v in st.items()), flush=True)


if __name__ == "__main__":
    main()
