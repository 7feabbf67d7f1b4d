"""`ListOpLog::encode_from(opts, from)` for a batch on the GPU (dtgpu_decode_encode_from, dt_patch.hip):
the `.dt` patch that takes a peer at `from` to the tip of a resident document.

The host encoder `ListOpLog.encode_from(o.dominators(req), opts)` on a host oplog of the same
document (pinned by test_encoder.py / test_gpu_encode.py) is the checker: every patch equals it
byte for byte, and the reduced request equals the host's dominators.  Golden text pins the meaning:
a device patch applied to the history at `from` rebuilds the document.  Every request has status 0
unless the test names the status it expects."""
import random

import pytest

import golden_data as G
from oracle.oracle import OpLog as OracleOpLog
from test_gpu_encode import _unicode_doc
from test_gpu_history import _backspaces, _dev_exact, _host_exact, _two_agents
import dt_amd

pytestmark = pytest.mark.gpu

ERR_CHECKOUT, ERR_ARG = 64, 67
WITH_CONTENT = dt_amd.EncodeOptions(True, False, False)
NO_CONTENT = dt_amd.EncodeOptions(False, True, False)
OPTION_SETS = [dt_amd.ENCODE_PATCH, WITH_CONTENT, NO_CONTENT]


def _host_patch(o, req, opts):
    return o.encode_from(o.dominators(req), opts)


def _check(base, hosts, docs, reqs, opts, expect=None):
    """One encode_from call; request i must have status expect[i] (0 when absent) -- the host
    encoder's own outcome -- and, with status 0, the host's frontier and bytes.  Returns the batch."""
    pb = base.encode_from(docs, reqs, opts)
    assert len(pb) == len(docs)
    for i, (d, req) in enumerate(zip(docs, reqs)):
        want = (expect or {}).get(i, 0)
        assert pb.status(i) == want, (i, req, pb.status(i))
        if want:
            with pytest.raises(dt_amd.ParseError) as e:
                pb.patch(i)
            assert e.value.code == want
            if want == ERR_CHECKOUT:
                with pytest.raises(dt_amd.ParseError) as e:
                    _host_patch(hosts[d], req, opts)
                assert e.value.code == ERR_CHECKOUT
            continue
        assert pb.frontier(i) == hosts[d].dominators(req), (i, req)
        assert pb.patch(i) == _host_patch(hosts[d], req, opts), (i, req)
    return pb


def _walk_doc():
    """pppp (a, ROOT, 0-3), qq (b, ROOT, 4-5), M (c, [3,5], 6), Y (a, [3], 7), Z (b, [6,7], 8) as a part
    plus three patches (a file is written in walk order and would renumber these)."""
    o = dt_amd.ListOpLog()
    a, b, c = (o.get_or_create_agent_id(n) for n in "abc")
    o.add_insert_at(a, [], 0, "pppp")
    o.add_insert_at(b, [], 0, "qq")
    part, f = o.encode(), o.local_frontier()
    patches = []
    for agent, parents, ch in ((c, [3, 5], "M"), (a, [3], "Y"), (b, [6, 7], "Z")):
        o.add_insert_at(agent, parents, 0, ch)
        patches.append(o.encode_from(f, dt_amd.ENCODE_PATCH))
        f = o.local_frontier()
    return o, part, patches


def test_walk_order():
    """The subset walk: a merge with no parent inside the patch is still deferred behind a
    non-merge; pieces inside an entry; the tip; a non-frontier request.  The base is a decode_add
    result."""
    built, part, patches = _walk_doc()
    host = dt_amd.ListOpLog.load_from(part)
    m = dt_amd.DecodeBatch([part])
    m.run()
    for p in patches:
        host.decode_and_add(p)
        m = m.add([p])
        assert m.add_result(0)[0] == 0
    for what in ("entries", "parents", "parent_offsets", "ops"):
        assert _host_exact(host)[what] == _host_exact(built)[what], what
    assert _dev_exact(m, 0) == _host_exact(host)
    assert _host_exact(host)["entries"] == [[0, 4], [4, 6], [6, 7], [7, 8], [8, 9]]
    reqs = [[3, 5], [3], [5], [1], [1, 5], [], [8], [3, 5, 1, 3]]
    pb = _check(m, {0: host}, [0] * len(reqs), reqs, WITH_CONTENT)
    got = [pb.patch(i) for i in range(len(reqs))]
    content = lambda s: bytes([13, 1 + len(s), 4]) + s   # a Content chunk: PlainText, the bytes
    # [3,5]: M has no parent inside the patch and is still a merge: Y goes first
    assert content(b"YMZ") in got[0] and content(b"MYZ") not in got[0]
    # [3]: walk qq, Y, M, Z; names in order of first mention; M's txn (1, foreign a:3, local 2 back)
    assert content(b"qqYMZ") in got[1]
    assert bytes([3, 6, 1]) + b"b" + bytes([1]) + b"a" + bytes([1]) + b"c" in got[1]
    assert bytes([23, 12, 2, 1, 1, 9, 3, 1, 11, 3, 8, 1, 6, 8]) in got[1]
    # [1]: the first piece starts inside the entry of pppp, its parent is LV 1
    assert pb.frontier(3) == [1] and content(b"ppYqqMZ") in got[3]
    assert bytes([23, 13, 2, 5, 1]) in got[3]   # txn pp: foreign parent a:1
    # [8], the tip: the empty patch, whose only agent name comes from the StartBranch version
    assert len(got[6]) == 35 and bytes([3, 2, 1]) + b"b" in got[6] and bytes([10, 4, 12, 2, 2, 2]) in got[6]
    # a non-frontier request reduces
    assert pb.frontier(7) == [3, 5] and got[7] == got[0]
    assert pb.last_ms > 0


def _mixed_doc():
    """test_gpu_history.test_mixed_known_and_unknown_content's document: one insert run whose
    content is known, then unknown, then known again."""
    o = dt_amd.ListOpLog()
    a = o.get_or_create_agent_id("seph")
    o.add_insert(a, 0, "abç")
    part, f = o.encode(), o.local_frontier()
    o.add_insert(a, 3, "déf")
    o.add_delete_without_content(a, 1, 3)
    o.add_insert(a, 1, "xy")
    p1, f = o.encode_from(f, NO_CONTENT), o.local_frontier()
    o.add_insert(a, 3, "ẑz!")
    p2 = o.encode_from(f, dt_amd.ENCODE_PATCH)
    return part, [p1, p2]


@pytest.fixture(scope="module")
def shapes():
    """The hand-made documents decoded once: (batch, host oplogs, status of the corrupted one)."""
    with_id = _two_agents()
    with_id.doc_id = "doc-ïd-42"
    tiny = dt_amd.ListOpLog()
    tiny.add_insert(tiny.get_or_create_agent_id("seph"), 0, "hi")
    back = _backspaces().encode()
    bad = bytearray(back)
    bad[-1] ^= 0xFF   # the checksum
    docs = [_unicode_doc(1).encode(), back, with_id.encode(), tiny.encode(), _backspaces().encode(NO_CONTENT), bytes(bad)]
    d = dt_amd.DecodeBatch(docs)
    d.run()
    hosts = {i: dt_amd.ListOpLog.load_from(x) for i, x in enumerate(docs[:5])}
    return d, hosts, d.status(5)["status"]


@pytest.mark.parametrize("opts", OPTION_SETS, ids=["patch", "uncompressed", "no_content"])
def test_hand_made_shapes(shapes, opts):
    d, hosts, want_bad = shapes
    assert want_bad != 0
    store = opts.store_inserted_content
    n1 = len(hosts[1])
    items = [
        (1, [3]), (0, [2]), (0, [40]),             # multi-byte inserts clipped by the piece start
        (1, [11]), (1, [12]), (1, [13]), (1, [10]),   # the reverse delete run cut at every interior LV
        (2, [3]), (2, [5]), (2, []),               # a doc id
        (3, []), (3, [0]), (0, []), (1, [1]),      # content below and above the 20-byte LZ4 cut
        (4, [3]), (4, [12]), (4, []),              # decoded without content
        (1, [n1]), (5, [3]), (1, [0, n1 - 1, 2]),  # an LV equal to n_lv; a corrupted base; doc[] repeats, out of order
    ]
    expect = {17: ERR_ARG, 18: want_bad}
    if store:   # the host raises where an insert without content is to be stored ([12] leaves deletes only)
        expect.update({14: ERR_CHECKOUT, 16: ERR_CHECKOUT})
    assert hosts[2].doc_id == "doc-ïd-42" and len(hosts[1]) == 15
    pb = _check(d, hosts, [i for i, _ in items], [v for _, v in items], opts, expect)
    if store:
        assert len(_host_patch(hosts[3], [], opts)) < 60 and b"hi" in pb.patch(10)
    assert b"doc-\xc3\xafd-42" in pb.patch(7)


@pytest.mark.parametrize("opts", OPTION_SETS, ids=["patch", "uncompressed", "no_content"])
def test_mixed_known_and_unknown_content(opts):
    part, patches = _mixed_doc()
    host = dt_amd.ListOpLog.load_from(part)
    m = dt_amd.DecodeBatch([part])
    m.run()
    for p in patches:
        host.decode_and_add(p)
        m = m.add([p])
    assert m.add_result(0)[0] == 0 and _dev_exact(m, 0) == _host_exact(host)
    assert m.status(0)["content_complete"] == 0
    reqs = [[], [1], [2], [4], [6], [9], [10], [12], [2, 11]]
    expect = {}
    if opts.store_inserted_content:   # the unknown inserts are LVs 3..9 (déf, xy and their deletes' neighbours)
        for i, v in enumerate(reqs):
            try:
                _host_patch(host, v, opts)
            except dt_amd.ParseError as e:
                assert e.code == ERR_CHECKOUT
                expect[i] = ERR_CHECKOUT
        assert sorted(expect) == [0, 1, 2, 3, 4], expect   # every request that leaves an unknown insert
    _check(m, {0: host}, [0] * len(reqs), reqs, opts, expect)


def test_start_branch_content_is_the_hosts():
    """ENCODE_FULL: a no-op for ROOT requests (the whole file), deferred for the others alone."""
    o = _unicode_doc(2)
    data = o.encode()
    host = dt_amd.ListOpLog.load_from(data)
    d = dt_amd.DecodeBatch([data])
    d.run()
    pb = d.encode_from([0, 0, 0], [[], [7], []], dt_amd.ENCODE_FULL)
    assert [pb.status(i) for i in range(3)] == [0, dt_amd.DECODE_DEFER, 0]
    assert pb.patch(0) == host.encode() and pb.patch(2) == host.encode() and pb.frontier(1) == [7]
    with pytest.raises(dt_amd.ParseError) as e:
        pb.patch(1)
    assert e.value.code == dt_amd.DECODE_DEFER
    with pytest.raises(dt_amd.ParseError) as e:
        d.encode_from([1], [[]])
    assert e.value.code == ERR_ARG


@pytest.fixture(scope="module")
def ff():
    data = G.dt_bytes("friendsforever")
    d = dt_amd.DecodeBatch([data])
    d.run()
    return data, dt_amd.ListOpLog.load_from(data), d


def _remote(o, lvs):
    names = [bytes(n) for n in o.export("agent_names")]
    return sorted((names[a], q) for a, q in (o.local_to_remote(x) for x in lvs))


def test_friendsforever(ff):
    data, o, d = ff
    n = len(o)
    assert n == 26078 and len(o.export("entries")) == 2405
    rng = random.Random(41)
    reqs = [rng.sample(range(n), k) for k in [1] * 16 + [2] * 8 + [3] * 4] + [[], o.local_frontier()]
    pb = _check(d, {0: o}, [0] * len(reqs), reqs, dt_amd.ENCODE_PATCH)
    want = G.trace("friendsforever_flat")["endContent"].encode()
    for i in (0, 17, 25, 28):   # a single LV, a pair, a triple, ROOT
        h = dt_amd.ListOpLog.load_from(o.history(reqs[i]).encode())
        f = h.decode_and_add(pb.patch(i))
        assert len(h) == n and _remote(h, f) == _remote(o, o.local_frontier()), i
        assert h.checkout_tip_bytes() == want, i


def test_the_loop_on_the_device(ff):
    """history -> encode_from -> add -> checkout, all on the device: each history plus its patch is
    the base document again."""
    rng = random.Random(43)
    docs = [ff[0], G.dt_bytes("git-makefile")] + [dt_amd.synth_merge_oplog(k, 3000).encode() for k in range(4)]
    want = [G.trace("friendsforever_flat")["endContent"].encode()]
    want += [OracleOpLog.load_from(x).checkout_tip_bytes() for x in docs[1:]]
    base = dt_amd.DecodeBatch(docs)
    base.run()
    idx = [0, 0, 1, 2, 3, 4, 5, 2, 0, 5]
    vs = [rng.sample(range(base.status(i)["n_lv"]), rng.choice([1, 2])) for i in idx]
    hist = base.history(idx, vs)
    pb = base.encode_from(idx, vs)
    assert [pb.status(i) for i in range(len(idx))] == [0] * len(idx)
    assert [pb.frontier(i) for i in range(len(idx))] == [hist.history_result(i)[1] for i in range(len(idx))]
    m = hist.add([pb.patch(i) for i in range(len(idx))])
    assert [m.add_result(i)[0] for i in range(len(idx))] == [0] * len(idx)
    b = m.checkout_batch()
    b.run()
    b.sync()
    res = b.results()
    for k, i in enumerate(idx):
        assert res[k]["status"] == 0, (k, res[k])
        assert b.text(k) == want[i], (k, vs[k])


def test_history_handle_as_base(ff):
    """A patch between two nested versions: the base is the history at the later one."""
    data, o, d = ff
    rng = random.Random(47)
    v2 = o.dominators(rng.sample(range(len(o)), 2))
    sub = o.history(v2)
    inside = rng.sample(range(len(sub)), 2)          # in the history's own numbering
    h = d.history([0], [v2])
    assert h.history_result(0) == (0, v2)
    _check(h, {0: sub}, [0, 0], [inside, []], dt_amd.ENCODE_PATCH)
    # the same version named in the base document's LVs maps onto it by (agent, seq)
    v1 = []
    for x in sub.dominators(inside):
        a, q = sub.local_to_remote(x)
        v1.append(o.remote_to_local(a, q)[0][0])
    mapped = [sub.remote_to_local(*o.local_to_remote(x))[0][0] for x in sorted(v1)]
    pb = h.encode_from([0], [mapped])
    assert pb.status(0) == 0 and pb.patch(0) == sub.encode_from(sub.dominators(mapped), dt_amd.ENCODE_PATCH)


def test_many_entries(monkeypatch):
    """2,423 entries and a tip frontier 8 wide.  The walk's scratch is in HBM at every size (one
    form); the mark sweep's words have the history projection's two forms, LDS and HBM scratch: both
    run here, through the projection's override."""
    data = dt_amd.synth_merge_oplog(0, 60000).encode()
    o = dt_amd.ListOpLog.load_from(data)
    assert len(o.export("entries")) == 2423
    rng = random.Random(53)
    reqs = [rng.sample(range(len(o)), rng.choice([1, 2, 3])) for _ in range(10)] + [o.local_frontier(), []]
    d = dt_amd.DecodeBatch([data])
    d.run()
    monkeypatch.setenv("DTGPU_HISTORY_LDS_ENTRIES", "0")
    pb = _check(d, {0: o}, [0] * 12, reqs, dt_amd.ENCODE_PATCH)
    assert all(pb.profile(i)[0] == 2 for i in range(12))
    monkeypatch.delenv("DTGPU_HISTORY_LDS_ENTRIES")
    pb = _check(d, {0: o}, [0] * 12, reqs, dt_amd.ENCODE_PATCH)
    assert all(pb.profile(i)[0] == 1 for i in range(12))
    assert pb.profile(11)[3] == 2423 and pb.profile(10)[3] == 0   # ROOT walks every entry, the tip none
