"""A plain Python restatement of the reference's version summaries (src/causalgraph/summary.rs):
summarize_versions (:119-132), intersect_with_summary_full (:175-208) and intersect_with_summary
(:234-264), over the exported arrays of an oplog (`agent_runs`, `agent_names`, `entries`,
`parent_offsets`, `parents`).  Dominators are found by brute-force reachability, so this is for
small documents only.  It shares no code with the engine: the host functions are compared with it,
and the device with the host functions."""


class Doc:
    """The arrays the model reads.  `src` is anything with export(what) (a host ListOpLog)."""

    def __init__(self, src):
        self.runs = [tuple(int(x) for x in r) for r in src.export("agent_runs")]   # lv, len, agent, seq
        self.names = [bytes(n) for n in src.export("agent_names")]
        self.entries = [tuple(int(x) for x in e) for e in src.export("entries")]
        self.poff = [int(x) for x in src.export("parent_offsets")]
        self.par = [int(x) for x in src.export("parents")]
        self.n_lv = self.entries[-1][1] if self.entries else 0

    def entry_of(self, lv):
        for k, (s, e) in enumerate(self.entries):
            if s <= lv < e:
                return k
        raise ValueError(lv)

    def parents_of(self, lv):
        k = self.entry_of(lv)
        return [lv - 1] if lv > self.entries[k][0] else self.par[self.poff[k]:self.poff[k + 1]]

    def history(self, lv):
        """Every LV that lv has seen, lv included."""
        seen, todo = set(), [lv]
        while todo:
            x = todo.pop()
            if x in seen:
                continue
            seen.add(x)
            todo.extend(self.parents_of(x))
        return seen

    def dominators(self, lvs):
        """find_dominators: the members that no other member has seen, ascending."""
        lvs = sorted(set(lvs))
        hist = {v: self.history(v) for v in lvs}
        return [v for v in lvs if not any(w != v and v in hist[w] for w in lvs)]


def summarize(doc):
    """[(name, [(start, end), ...])] per agent with ops, in agent-id order; ranges sorted and merged
    where adjacent (merge_spans)."""
    out = []
    for a, name in enumerate(doc.names):
        spans = sorted((seq, seq + ln) for _lv, ln, agent, seq in doc.runs if agent == a)
        merged = []
        for s, e in spans:
            if merged and merged[-1][1] == s:
                merged[-1] = (merged[-1][0], e)
            else:
                merged.append((s, e))
        if merged:
            out.append((name, merged))
    return out


def pieces(doc, summary):
    """intersect_with_summary_full's visits: (entry index, start, end, base LV of the piece | None)
    in visiting order.  `summary` is [(name bytes, [(start, end), ...])]."""
    out = []
    for k, (name, ranges) in enumerate(summary):
        agent = doc.names.index(name) if name in doc.names else None
        runs = sorted((seq, ln, lv) for lv, ln, a, seq in doc.runs if a == agent) if agent is not None else []
        for s, e in ranges:
            assert s < e
            nxt = s
            for seq, ln, lv in runs:
                ps, pe = max(s, seq), min(e, seq + ln)
                if ps >= pe:
                    continue
                if ps > nxt:
                    out.append((k, nxt, ps, None))
                out.append((k, ps, pe, lv + (ps - seq)))
                nxt = pe
            if nxt < e:
                out.append((k, nxt, e, None))
    return out


def intersect(doc, summary, frontier=()):
    """(common frontier, remainder records (entry index, start, end)) -- records, not yet grouped
    by name: group() does that."""
    versions, rem = [int(v) for v in frontier], []
    for k, s, e, base in pieces(doc, summary):
        if base is None:
            rem.append((k, s, e))
        else:
            versions.append(base + (e - s) - 1)
    assert all(v < doc.n_lv for v in versions)
    return doc.dominators(versions), rem


def group(summary, records):
    """The remainder as the reference builds it (:246-255): consecutive records of equal name merge
    into one entry; None when there is none."""
    out = []
    for k, s, e in records:
        name = summary[k][0].decode()
        if out and out[-1][0] == name:
            out[-1][1].append((s, e))
        else:
            out.append((name, [(s, e)]))
    return out or None
