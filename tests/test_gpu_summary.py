"""`CausalGraph::intersect_with_summary` for a batch on the GPU (dtgpu_decode_intersect,
dtgpu_decode_encode_from_summaries, dt_summary.hip): a peer's version summary met with a resident
document gives the common frontier, the remainder and the `.dt` patch of what the peer lacks.

The host functions (dtgpu_oplog_intersect_summary / dtgpu_oplog_summarize, pinned against the
reference's vectors and a model of summary.rs by test_summary_api.py) on a host oplog of the same
document are the checker: request for request the device's status, frontier and remainder records
equal theirs.  Shapes are the smallest that cross the kernel's 64-lane steps in every dimension it
spreads over lanes."""
import random

import pytest

import golden_data as G
import summary_docs as D
import dt_amd

pytestmark = pytest.mark.gpu

ERR_ARG = 67


def _resident(files):
    d = dt_amd.DecodeBatch(files)
    d.run()
    return d


def _loaded(oplogs):
    """(host oplogs, resident batch) of the same `.dt` bytes: a file is written in walk order, so LVs
    are read off what was loaded, never off the oplog that wrote it."""
    files = [o.encode() for o in oplogs]
    return [dt_amd.ListOpLog.load_from(f) for f in files], _resident(files)


def _check(base, hosts, docs, summaries, frontiers=None, expect=None, sync=False):
    """One intersect call (or the fused call); request i must have the host's status -- expect[i],
    0 when absent -- and with status 0 the host's frontier and remainder records."""
    if sync:
        pb, x = base.sync(docs, summaries, frontiers=frontiers)
    else:
        pb, x = None, base.intersect(docs, summaries, frontiers)
    assert len(x) == len(docs)
    for i, (d, sm) in enumerate(zip(docs, summaries)):
        f = frontiers[i] if frontiers is not None else ()
        want = (expect or {}).get(i, 0)
        if hosts[d] is not None:
            st, hf, hrec = hosts[d].intersect_summary_records(sm, f)
            assert st == want, (i, st, want)
        assert x.status(i) == want, (i, x.status(i), want)
        if want:
            assert x.frontier(i) == [] and x.remainder_records(i) == []
            continue
        assert x.frontier(i) == hf, (i, sm)
        assert x.remainder_records(i) == hrec, (i, sm)
        assert x.remainder(i) == hosts[d].intersect_with_summary(sm, f)[1]
        if pb is not None:
            assert pb.status(i) == 0 and pb.frontier(i) == hf
            assert pb.patch(i) == hosts[d].encode_from(hf, dt_amd.ENCODE_PATCH), i
    return (pb, x) if sync else x


def test_reference_vectors():
    """summary.rs `summary_smoke` and `intersect_summary`, the values as test_summary_api.py has them."""
    before, after = D.smoke_doc()
    sparse = D.sparse_doc()
    kaarina, v = D.sparse_doc_with_kaarina()
    hosts, base = _loaded([before, after, sparse, kaarina])
    for i, h in enumerate(hosts):
        assert base.status(i)["status"] == 0
        assert base.summarize_versions(i) == h.summarize_versions()
    assert base.summarize_versions(1) == [("seph", [(0, 10)]), ("mike", [(0, 5), (15, 20)])]
    assert base.summarize_versions(2) == [("seph", [(1, 5), (8, 9)])]
    kv = len(hosts[3]) - 1
    x = _check(base, hosts, [0, 1, 2, 3, 2, 2], [D.REF_VS, after.summarize_versions(), D.REF_VS, D.REF_VS, [], []],
               [[9], [], [], [kv], [], [2, 2, 0]])
    assert x.remainder(2) == [("seph", [(0, 1), (5, 8), (9, 10)]), ("mike", [(0, 5)])]
    assert len(x.frontier(2)) == 2
    assert x.frontier(3) == [kv] and x.frontier(4) == [] and x.remainder(4) is None
    assert x.last_ms > 0 and x.profile(2)[:3] == [2, 4, 0]


def test_runs_out_of_seq_order():
    """One agent's runs where LV order != seq order (a later span merged first), and the same with
    a span that never arrives: the pieces of a range are ranked before its gaps are cut."""
    files, hosts = [], []
    for sparse in (False, True):
        part, patch = D.reordered_parts(sparse)
        files.append((part, patch))
        hosts.append(D.reordered_host(sparse))
    base = _resident([p for p, _ in files]).add([q for _, q in files])
    for i in (0, 1):
        assert base.add_result(i)[0] == 0
        assert [list(map(int, r)) for r in base.export(i, "agent_runs")] == \
            [list(map(int, r)) for r in hosts[i].export("agent_runs")]
        assert base.summarize_versions(i) == hosts[i].summarize_versions()
    sms = [[("x", [(2, 13)]), ("x", [(0, 20)]), ("y", [(1, 5)])], [("x", [(0, 15)])], [("x", [(7, 8), (1, 2)])]]
    x = _check(base, hosts, [0, 0, 0, 1, 1, 1], sms + sms)
    assert x.profile(0)[2] == 2 and x.profile(3)[2] == 2 and x.profile(2)[2] == 0
    assert x.remainder(3) == [("x", [(5, 10), (5, 10), (15, 20)]), ("y", [(2, 5)])]
    _check(base, hosts, [0, 1], [sms[0], sms[0]], sync=True)


def test_every_lane_dimension_crosses_64():
    # 70 agents (wide_docs' names); 140 agent runs of two agents
    hosts, base = _loaded([D.many_agents_doc(70), D.alternating_doc(70, 2)])
    fan = hosts[0]
    assert base.status(0)["n_agents"] == 70 and base.status(1)["n_aruns"] == 140
    for i in (0, 1):
        assert base.summarize_versions(i) == hosts[i].summarize_versions()
    names = [bytes(n).decode() for n in fan.export("agent_names")]
    docs, sms = [], []
    # agents past the first 64 of the table, by name; prefixes and extensions of names are unknown
    docs.append(0)
    sms.append([(names[66], [(0, 5)]), (names[64], [(1, 2)]), (names[0], [(0, 100)]), (names[65][:-1], [(0, 2)]),
                (names[65] + "0", [(0, 2)]), (names[69], [(3, 4)]), (names[63], [(0, 4)])])
    # every run of ann: 70 known pieces in one range; a piece on each side of the 64-run step
    docs.append(1)
    sms.append([("ann", [(0, 140)]), ("bob", [(125, 131)]), ("ann", [(127, 129)])])
    # 70 ranges in one entry, each clipping a run to its last seq; ranges across runs; 70 remainder
    # records from the 70 ranges of one entry
    docs.append(1)
    sms.append([("ann", [(2 * k + 1, 2 * k + 2) for k in range(70)]), ("bob", [(3 * k, 3 * k + 2) for k in range(70)]),
                ("bob", [(200 + 2 * k, 201 + 2 * k) for k in range(70)])])
    # 70 entries in one request, known and unknown names alternating
    docs.append(1)
    sms.append([(("ann", "carl", "bob")[k % 3], [(k, k + 3)]) for k in range(70)])
    # 70 remainder records from one range each, then known ones
    docs.append(1)
    sms.append([("dora", [(k, k + 1)]) for k in range(70)] + [("bob", [(139, 1 << 40)])])
    x = _check(base, hosts, docs, sms)
    assert x.profile(1)[0] == 70 + 4 + 2 and len(x.remainder_records(2)) >= 70 and len(x.remainder_records(4)) == 71
    assert x.remainder_records(4)[-1] == (70, 140, 1 << 40)
    _check(base, hosts, docs, sms, sync=True)


def test_batch_mechanics():
    """Requests repeating a document, several documents, a corrupt one, a bad range and a bad extra
    LV failing alone; merged and history handles as the base."""
    sparse = D.sparse_doc()
    before, after = D.smoke_doc()
    bad = bytearray(after.encode())
    bad[-1] ^= 0xFF   # the checksum
    files = [sparse.encode(), before.encode(), bytes(bad)]
    hosts = [dt_amd.ListOpLog.load_from(files[0]), dt_amd.ListOpLog.load_from(files[1]), None]
    base = _resident(files)
    want_bad = base.status(2)["status"]
    assert want_bad != 0
    docs = [1, 0, 2, 0, 0, 1, 0, 1]
    sms = [D.REF_VS, D.REF_VS, D.REF_VS, [("seph", [(1, 3), (4, 4)])], D.REF_VS, after.summarize_versions(), [], D.REF_VS]
    frs = [[], [], [], [], [len(hosts[0])], [3], [], [14, 2, 14]]
    x = _check(base, hosts, docs, sms, frs, expect={2: want_bad, 3: ERR_ARG, 4: ERR_ARG})
    assert x.remainder(5) == [("mike", [(15, 20)])]
    pb, x = _check(base, hosts, docs, sms, frs, expect={2: want_bad, 3: ERR_ARG, 4: ERR_ARG}, sync=True)
    for i, st in ((2, want_bad), (3, ERR_ARG), (4, ERR_ARG)):
        assert pb.status(i) == st
    # the start-branch content of a non-ROOT request stays with the host encoder, as in encode_from;
    # the intersection of that request stands
    pb, x = base.sync([0, 0], [D.REF_VS, []], dt_amd.ENCODE_FULL)
    assert pb.status(0) == dt_amd.DECODE_DEFER and x.status(0) == 0 and x.frontier(0) == hosts[0].intersect_with_summary(D.REF_VS)[0]
    assert pb.status(1) == 0 and pb.patch(1) == hosts[0].encode_from([], dt_amd.ENCODE_FULL)
    # a merged handle: before + the patch to after
    grown = dt_amd.ListOpLog.load_from(files[1])
    patch = after.encode()
    grown.decode_and_add(patch)
    m = _resident([files[1]]).add([patch])
    assert m.add_result(0)[0] == 0 and m.summarize_versions(0) == grown.summarize_versions()
    _check(m, [grown], [0, 0], [after.summarize_versions(), D.REF_VS], sync=True)
    # a history handle: `after` without mike's last span is `before` again
    h = m.history([0], [hosts[1].local_frontier()])
    assert h.history_result(0)[0] == 0 and h.summarize_versions(0) == hosts[1].summarize_versions()
    _check(h, [hosts[1]], [0, 0], [after.summarize_versions(), []], sync=True)
    # no requests at all
    assert len(base.intersect([], [])) == 0


@pytest.fixture(scope="module")
def ff():
    data = G.dt_bytes("friendsforever")
    return dt_amd.ListOpLog.load_from(data), _resident([data])


def test_friendsforever_versions(ff):
    o, base = ff
    rng = random.Random(11)
    versions = [0, len(o) - 1] + [rng.randrange(len(o)) for _ in range(30)]
    peers = [o.history([v]) for v in versions]
    hellos = [c.summarize_versions() for c in peers]
    docs = [0] * len(versions)
    x = base.intersect(docs, hellos)
    pb, x2 = base.sync(docs, hellos)
    fronts = [o.dominators([v]) for v in versions]
    two_call = base.encode_from(docs, [x.frontier(i) for i in range(len(versions))])
    for i, v in enumerate(versions):
        assert x.status(i) == 0 and x.frontier(i) == fronts[i] and x.remainder(i) is None, v
        assert x2.status(i) == 0 and x2.frontier(i) == fronts[i] and x2.remainder(i) is None, v
        assert pb.status(i) == 0 and pb.frontier(i) == fronts[i]
        assert pb.patch(i) == o.encode_from(fronts[i], dt_amd.ENCODE_PATCH), v
        assert pb.patch(i) == two_call.patch(i), v
    gold = G.trace("friendsforever_flat")["endContent"].encode()
    for i in (0, 5, 17):
        c = peers[i]
        c.decode_and_add(pb.patch(i))
        assert c.summarize_versions() == o.summarize_versions()
        assert c.checkout_tip_bytes() == gold
    assert base.summarize_versions(0) == o.summarize_versions()


def test_a_peer_that_is_ahead(ff):
    """The peer holds further seqs of the agents the server knows and ops by a new agent: the
    remainder is exactly those ranges, and the patch is what it would be without them (empty)."""
    o, _ = ff
    (server,), base = _loaded([o.history([len(o) // 3])])
    peer = dt_amd.ListOpLog.load_from(o.encode())
    peer.add_insert(peer.get_or_create_agent_id("zed"), 0, "new agent")
    have, hello = dict(server.summarize_versions()), peer.summarize_versions()
    pb, x = base.sync([0], [hello])
    assert x.status(0) == 0 and x.frontier(0) == server.local_frontier()
    assert x.remainder(0) == [(n, [(have[n][-1][1], rs[-1][1])]) for n, rs in hello[:2]] + [("zed", [(0, 9)])]
    assert (x.frontier(0), x.remainder(0)) == server.intersect_with_summary(hello)
    assert pb.patch(0) == server.encode_from(server.local_frontier(), dt_amd.ENCODE_PATCH)
    assert pb.patch(0) == base.sync([0], [server.summarize_versions()])[0].patch(0)


def test_random_summaries_against_the_host():
    """Random summaries (summary_docs.random_summary: unknown names, prefixes, clipped runs, 2^40,
    duplicates) over small concurrent documents, one batch."""
    rng = random.Random(5)
    hosts, base = _loaded([dt_amd.synth_merge_oplog(k, 250) for k in range(3)])
    assert [base.status(i)["status"] for i in range(3)] == [0, 0, 0]
    docs = [rng.randrange(3) for _ in range(90)]
    sms = [D.random_summary(rng, hosts[d]) for d in docs]
    frs = [D.random_frontier(rng, hosts[d]) for d in docs]
    _check(base, hosts, docs, sms, frs)
    _check(base, hosts, docs[:30], sms[:30], frs[:30], sync=True)
