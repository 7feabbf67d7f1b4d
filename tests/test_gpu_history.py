"""`ListOpLog::checkout(&[LV])` for a batch, up to the replay (dtgpu_decode_history, dt_history.hip):
the history of a version of a resident document, built on the GPU as an oplog of its own.

The host's history sub-oplog (dtgpu_oplog_history; pinned against the oracle by
tests/test_checkout_version.py) is the checker: every exported array of every output equals the
host's element for element -- the same RLE runs, agent names kept, no doc id -- and the reduced
request equals the host's dominators.  The projected batches then check out on the device against
the oracle's checkout at the same versions."""
import random

import numpy as np
import pytest

import golden_data as G
from oracle.oracle import OpLog as OracleOpLog
import dt_amd

pytestmark = pytest.mark.gpu

ARRAYS = ("ops", "agent_runs", "entries", "parent_offsets", "parents", "content", "char_offsets", "version")
ERR_ARG = 67
NONE = 0xFFFFFFFF


def _host_exact(o):
    out = {"names": [bytes(n) for n in o.export("agent_names")], "doc_id": o.doc_id}
    for what in ARRAYS:
        out[what] = np.asarray(o.export(what)).tolist()
    return out


def _dev_exact(m, i):
    out = {"names": [bytes(n) for n in m.export(i, "agent_names")], "doc_id": m.doc_id(i)}
    for what in ARRAYS:
        out[what] = np.asarray(m.export(i, what)).tolist()
    return out


def _project(items):
    """items: (document bytes, version).  One DecodeBatch over the distinct documents (decoded on the
    device), one history call; returns (decoded batch, history batch, document index of each item)."""
    docs, idx = [], []
    for data, _ in items:
        if data not in docs:
            docs.append(data)
        idx.append(docs.index(data))
    d = dt_amd.DecodeBatch(docs)
    d.run()
    h = d.history(idx, [v for _, v in items])
    assert len(h) == len(items)
    return d, h, idx


def _check(items, hosts=None):
    """Every output has status 0 (no deferral), equals the host's history array for array, and its
    reduced request equals the host's dominators.  hosts: document bytes -> host oplog (loaded when
    absent).  Returns the same as _project."""
    hosts = dict(hosts or {})
    d, h, idx = _project(items)
    for i, (data, v) in enumerate(items):
        if data not in hosts:
            hosts[data] = dt_amd.ListOpLog.load_from(data)
        full = hosts[data]
        st, f = h.history_result(i)
        assert st == 0 and st != dt_amd.DECODE_DEFER, (i, st)
        assert h.status(i)["status"] == 0, i
        assert f == full.dominators(v), (i, v)
        assert _dev_exact(h, i) == _host_exact(full.history(v)), (i, v)
    return d, h, idx


def _two_agents():
    o = dt_amd.ListOpLog()
    a, b = o.get_or_create_agent_id("a"), o.get_or_create_agent_id("b")
    o.add_insert_at(a, [], 0, "aaaa")
    o.add_insert_at(b, [], 0, "bb")
    o.add_insert_at(a, [3], 4, "cccc")
    return o


def _backspaces():
    o = dt_amd.ListOpLog()
    a = o.get_or_create_agent_id("seph")
    o.add_insert(a, 0, "héllo wörld")
    for p in (10, 9, 8, 7):
        o.add_delete_without_content(a, p, p + 1)
    return o


def test_hand_made_shapes():
    """The cross-gap merges, clipped multi-byte inserts and reverse delete runs, a document without
    content, ROOT, the tip, non-frontier requests, an LV out of range and a corrupted base, in one
    batch."""
    two = _two_agents().encode()
    back = _backspaces().encode()
    bare = _backspaces().encode(dt_amd.EncodeOptions(False, False, False))
    ff = G.dt_bytes("friendsforever")
    full = dt_amd.ListOpLog.load_from(ff)
    bad = bytearray(back)
    bad[-1] ^= 0xFF   # the checksum
    bad = bytes(bad)
    good = [(two, [9]), (back, [3]), (back, [12]), (back, [13]), (bare, [12]), (ff, []), (two, []),
            (ff, full.local_frontier()), (back, [14]), (ff, [3, 9]), (ff, [9, 9]), (two, [5, 9, 3])]
    d, h, idx = _check(good)
    # (a) one entry, one op run, one agent run across the skipped concurrent insert; both names
    # kept.  (A file is written in walk order, which would put "cccc" right after "aaaa": the
    # document arrives as a part plus a patch, which keeps its LV order, so the base is a merged handle.)
    src = _two_agents()
    o = dt_amd.ListOpLog()
    o.get_or_create_agent_id("a"), o.get_or_create_agent_id("b")
    o.add_insert_at(0, [], 0, "aaaa")
    o.add_insert_at(1, [], 0, "bb")
    part, f = o.encode(), o.local_frontier()
    o.add_insert_at(0, [3], 4, "cccc")
    patch = o.encode_from(f, dt_amd.ENCODE_PATCH)
    d2 = dt_amd.DecodeBatch([part])
    d2.run()
    m = d2.add([patch])
    assert m.add_result(0)[0] == 0 and _dev_exact(m, 0) == _host_exact(src)
    h2 = m.history([0, 0], [[9], [9, 5]])
    assert h2.history_result(0) == (0, [9]) and h2.history_result(1) == (0, [5, 9])
    assert _dev_exact(h2, 1) == _host_exact(src.history([5, 9]))
    a = _dev_exact(h2, 0)
    assert a == _host_exact(src.history([9]))
    assert a["entries"] == [[0, 8]] and a["ops"] == [[0, 8, 0, 2]] and a["agent_runs"] == [[0, 8, 0, 0]]
    assert a["version"] == [7] and bytes(a["content"]) == b"aaaacccc" and a["names"] == [b"a", b"b"]
    assert a["parent_offsets"] == [0, 0] and a["parents"] == []
    # (b) a clipped multi-byte insert; reverse delete runs clipped from the right
    assert _dev_exact(h, 1)["char_offsets"] == [0, 1, 3, 4]
    assert _dev_exact(h, 2)["ops"][-1] == [11, 2, 9, 1]
    assert _dev_exact(h, 3)["ops"][-1] == [11, 3, 8, 1]
    # (c) no inserted content: the offsets stay ~0
    c = _dev_exact(h, 4)
    assert c["char_offsets"] == [NONE] * 13 and c["content"] == [] and h.status(4)["content_complete"] == 0
    # (d) ROOT: zero LVs, empty arrays
    for i in (5, 6):
        r = _dev_exact(h, i)
        assert h.status(i)["n_lv"] == 0 and all(r[w] == [] for w in ARRAYS if w != "parent_offsets")
        assert r["parent_offsets"] == [0] and h.history_result(i) == (0, [])
    # (e) the tip is the base document again (but for the doc id)
    for i in (7, 8):
        tip, base = _dev_exact(h, i), _dev_exact(d, idx[i])
        tip.pop("doc_id"), base.pop("doc_id")
        assert tip == base
    # (f) non-frontier requests reduce
    assert h.history_result(9) == (0, [9]) and h.history_result(10) == (0, [9])
    assert all(h.profile(i)[0] == 1 for i in range(len(good)))   # the per-entry words were in LDS
    # (g) an LV equal to n_lv and (h) a corrupted base fail alone
    mixed = [(back, [3]), (back, [15]), (bad, [3]), (two, [9]), (ff, [len(full)]), (ff, [100])]
    d, h, idx = _project(mixed)
    want_bad = d.status(idx[2])["status"]
    assert want_bad != 0
    with pytest.raises(dt_amd.ParseError) as e:
        dt_amd.ListOpLog.load_from(bad)
    assert e.value.code == want_bad
    assert [h.history_result(i)[0] for i in range(6)] == [0, ERR_ARG, want_bad, 0, ERR_ARG, 0]
    hosts = {back: dt_amd.ListOpLog.load_from(back), two: dt_amd.ListOpLog.load_from(two), ff: full}
    for i in (0, 3, 5):
        data, v = mixed[i]
        assert _dev_exact(h, i) == _host_exact(hosts[data].history(v)), i
    for i in (1, 2, 4):
        assert h.status(i)["status"] != 0 and len(h.export(i, "ops")) == 0


def test_mixed_known_and_unknown_content():
    """One insert run whose content is known, then unknown (a patch stored without content), then
    known again: the op run stays whole, the content and offsets keep the known chars only."""
    o = dt_amd.ListOpLog()
    a = o.get_or_create_agent_id("seph")
    o.add_insert(a, 0, "abç")
    part, f = o.encode(), o.local_frontier()
    o.add_insert(a, 3, "déf")
    o.add_delete_without_content(a, 1, 3)
    o.add_insert(a, 1, "xy")
    p1, f = o.encode_from(f, dt_amd.EncodeOptions(False, False, False)), o.local_frontier()
    o.add_insert(a, 3, "ẑz!")
    p2 = o.encode_from(f, dt_amd.ENCODE_PATCH)
    host = dt_amd.ListOpLog.load_from(part)
    host.decode_and_add(p1)
    host.decode_and_add(p2)
    d = dt_amd.DecodeBatch([part])
    d.run()
    m = d.add([p1]).add([p2])
    assert m.add_result(0)[0] == 0 and _dev_exact(m, 0) == _host_exact(host)
    assert _host_exact(host)["char_offsets"][2:11] == [2] + [NONE] * 7 + [4]
    vs = [[1], [4], [6], [9], [10], [12], [2, 11], []]
    h = m.history([0] * len(vs), vs)
    for i, v in enumerate(vs):
        assert h.history_result(i) == (0, host.dominators(v)), v
        assert _dev_exact(h, i) == _host_exact(host.history(v)), v
        assert h.status(i)["content_complete"] == (1 if not v or max(v) < 3 else 0), v


def test_friendsforever_random_versions_and_checkout():
    data = G.dt_bytes("friendsforever")
    full = dt_amd.ListOpLog.load_from(data)
    ora = OracleOpLog.load_from(data)
    rng = random.Random(21)
    vs = [rng.sample(range(len(full)), rng.choice([1, 2, 3])) for _ in range(16)]
    _, h, _ = _check([(data, v) for v in vs], {data: full})
    fronts = [h.history_result(i)[1] for i in range(16)]
    b = h.checkout_batch()
    b.run()
    b.sync()
    res = b.results()
    for i, f in enumerate(fronts):
        assert res[i]["status"] == 0, (i, res[i])
        assert b.text(i) == ora.checkout_bytes(f), (i, vs[i])


def _oracle_rebuild(sub):
    """Rebuild an engine oplog in the oracle one LV at a time (same agents, parents, positions)."""
    names = sub.export("agent_names")
    ora = OracleOpLog()
    ids = [ora.agent(n.decode() if isinstance(n, bytes) else n) for n in names]
    ents = sub.export("entries").reshape(-1, 2)
    off = sub.export("parent_offsets")
    par = sub.export("parents")
    content = bytes(sub.export("content"))
    coff = sub.export("char_offsets")
    agent_of = {}
    for lv, ln, agent, _seq in sub.export("agent_runs").reshape(-1, 4):
        for k in range(int(ln)):
            agent_of[int(lv) + k] = ids[int(agent)]
    parents_of = {}
    for i, (s, e) in enumerate(ents):
        parents_of[int(s)] = [int(x) for x in par[off[i]:off[i + 1]]]
    for lv, ln, pos, kf in sub.export("ops").reshape(-1, 4):
        lv, ln, pos, kind, fwd = int(lv), int(ln), int(pos), int(kf) & 1, (int(kf) >> 1) & 1
        for k in range(ln):
            v = lv + k
            ps = parents_of.get(v, [v - 1])
            if kind == 0:
                b = int(coff[v])
                ch = content[b:b + 4].decode("utf-8", errors="ignore")[:1]
                ora.add_insert_at(agent_of[v], ps, pos + k, ch)
            else:
                p = pos if fwd else pos + ln - 1 - k
                ora.add_delete_at(agent_of[v], ps, p, p + 1)
    return ora


def test_mixed_batch():
    """Documents of very different sizes, document indices shuffled and repeated: three versions of
    git-makefile, one mid-history version of node_nodecc, four each of two synthetic documents."""
    rng = random.Random(23)
    items, oracles, hosts = [], {}, {}
    for name, k in (("git-makefile", 3), ("node_nodecc", 1)):
        data = G.dt_bytes(name)
        hosts[data] = dt_amd.ListOpLog.load_from(data)
        oracles[data] = OracleOpLog.load_from(data)
        n = len(hosts[data])
        items += [(data, [n // 2] if k == 1 else [rng.randrange(n)]) for _ in range(k)]
    for doc in range(2):
        data = dt_amd.synth_oplog(doc, 2000).encode()
        o = dt_amd.ListOpLog.load_from(data)   # (a file is written in walk order: its own LV numbering)
        hosts[data] = o
        oracles[data] = _oracle_rebuild(o)
        items += [(data, sorted(rng.sample(range(len(o)), rng.choice([1, 2])))) for _ in range(4)]
    rng.shuffle(items)
    _, h, _ = _check(items, hosts)
    fronts = [h.history_result(i)[1] for i in range(len(items))]
    b = h.checkout_batch()
    b.run()
    b.sync()
    res = b.results()
    for i, (data, v) in enumerate(items):
        assert res[i]["status"] == 0, (i, res[i])
        assert b.text(i) == oracles[data].checkout_bytes(fronts[i]), (i, v)


def test_many_entries_wide_frontiers(monkeypatch):
    """A wide synthetic history (a tip frontier 8 wide; 2,423 entries once its file is loaded) with
    the per-entry mark words in HBM scratch: the LDS form would hold them (up to 12,288 entries),
    so DTGPU_HISTORY_LDS_ENTRIES forces the other one; then the same requests in LDS."""
    data = dt_amd.synth_merge_oplog(0, 60000).encode()
    o = dt_amd.ListOpLog.load_from(data)
    rng = random.Random(27)
    vs = [o.local_frontier()] + [rng.sample(range(len(o)), rng.choice([2, 3])) for _ in range(4)]
    assert len(vs[0]) == 8 and len(o.export("entries")) == 2423
    monkeypatch.setenv("DTGPU_HISTORY_LDS_ENTRIES", "0")
    _, h, _ = _check([(data, v) for v in vs], {data: o})
    assert all(h.profile(i)[0] == 2 for i in range(len(vs)))
    monkeypatch.delenv("DTGPU_HISTORY_LDS_ENTRIES")
    _, h, _ = _check([(data, v) for v in vs[:2]], {data: o})
    assert h.profile(0)[0] == 1 and h.profile(1)[0] == 1


def test_chaining():
    """A history handle is a base for decode_and_add (the patch from that version rebuilds the
    document) and for a further history."""
    data = G.dt_bytes("friendsforever")
    full = dt_amd.ListOpLog.load_from(data)
    rng = random.Random(29)
    vs = [full.dominators(rng.sample(range(len(full)), k)) for k in (1, 2)]
    _, h, _ = _check([(data, v) for v in vs], {data: full})
    patches = [full.encode_from(v, dt_amd.ENCODE_PATCH) for v in vs]
    m = h.add(patches)
    hosts = [full.history(v) for v in vs]
    for i, v in enumerate(vs):
        st, f = m.add_result(i)
        hf = hosts[i].decode_and_add(patches[i])
        assert st == 0 and sorted(f) == sorted(hf), i
        assert _dev_exact(m, i) == _host_exact(hosts[i]), i
    # the history of a history handle, at versions of its own numbering
    subs = [full.history(v) for v in vs]
    v2 = [rng.sample(range(len(s)), 2) for s in subs]
    h2 = h.history([0, 1, 1], [v2[0], v2[1], []])
    for i, (k, v) in enumerate([(0, v2[0]), (1, v2[1]), (1, [])]):
        st, f = h2.history_result(i)
        assert st == 0 and f == subs[k].dominators(v), i
        assert _dev_exact(h2, i) == _host_exact(subs[k].history(v)), i
    b = m.checkout_batch()
    b.run()
    want = G.trace("friendsforever_flat")["endContent"].encode()
    assert b.text(0) == want and b.text(1) == want


def test_checkout_versions():
    data = G.dt_bytes("friendsforever")
    full = dt_amd.ListOpLog.load_from(data)
    rng = random.Random(31)
    vs = [[]] + [rng.sample(range(len(full)), rng.choice([1, 2, 3])) for _ in range(6)] + [full.local_frontier()]
    d = dt_amd.DecodeBatch([data])
    d.run()
    got = d.checkout_versions([0] * len(vs), vs)
    assert len(got) == 8
    for br, v in zip(got, vs):
        want = full.checkout(v)
        assert br.content_bytes() == want.content_bytes(), v
        assert br.local_frontier() == want.local_frontier(), v
    assert got[0].content_bytes() == b"" and got[0].local_frontier() == []
    with pytest.raises(dt_amd.ParseError):
        d.checkout_versions([0], [[len(full)]])
