"""Batched `ListOpLog::iter_xf_operations_from` / `ListBranch::merge` over resident documents
(dtgpu_decode_xf_from; DecodeBatch.xf_operations_from / merge): projection, prep, plan_kernel_xf and
the transformed-ops replay, all on the device.

The checker is the host path on a host oplog loaded from the same `.dt` bytes: for every request
ListOpLog.xf_operations_lv(a, b) (dtgpu_xf_operations_from: host plan, one staged batch per call),
dominators(a, b), the oracle's checkout_bytes of that frontier and, on the named fixtures and the
small document, the oracle's xf_operations_from.  A file is written in walk order, so every LV here
is read off the loaded oplog."""
import random

import pytest

import golden_data as G
import merge_docs as M
import wide_docs as W
from oracle.oracle import OpLog as OracleOpLog, oplog_from_trace as oracle_from_trace
import dt_amd

pytestmark = pytest.mark.gpu

ERR_ARG = 67
DEFER = dt_amd.DECODE_DEFER


class Doc:
    """A document's bytes with its checkers: the host oplog and the oracle, loaded from them."""

    def __init__(self, data):
        self.data = bytes(data)
        self.host = dt_amd.ListOpLog.load_from(self.data)
        self.ora = OracleOpLog.load_from(self.data)
        self._text = {}

    def text_at(self, frontier):
        k = tuple(frontier)
        if k not in self._text:
            self._text[k] = self.ora.checkout_bytes(list(frontier))
        return self._text[k]


def _resident(docs):
    d = dt_amd.DecodeBatch([x.data for x in docs])
    d.run()
    return d


def _check(m, i, doc, a, b, oracle=True, host=True):
    """Request i of MergeBatch m is (a -> b) on `doc`: status, version, records, content."""
    assert m.status(i) == 0, (i, a, b, m.status(i))
    front = doc.host.dominators(a, b)
    assert m.version(i) == front, (i, a, b)
    got = m.xf_operations_lv(i)
    if host:
        assert got == doc.host.xf_operations_lv(a, b), (i, a, b)
    if oracle:
        assert got == M.oracle_records(doc.ora, a, b), (i, a, b)
    assert m.content_bytes(i) == doc.text_at(front), (i, a, b)
    return got


# ---- 1. the small document, every ordered pair of its versions, in one call ----------------------

def test_small_document_every_pair_in_one_call():
    doc = Doc(M.small_bytes())
    pairs = M.all_pairs(doc.host)
    assert len(pairs) == 1444
    d = _resident([doc])
    m = d.xf_operations_from([0] * len(pairs), [a for a, _ in pairs], [b for _, b in pairs])
    assert len(m) == 1444
    already = 0
    ex = M.exports(doc.host)
    for i, (a, b) in enumerate(pairs):
        got = _check(m, i, doc, a, b)
        already += sum(1 for _lv, x in got if x is None)
        # the stream takes the checkout at `from` to the checkout at the merged version
        assert M.apply(doc.text_at(a).decode(), M.per_char(ex, got)).encode() == m.content_bytes(i)
    assert already == 245


# ---- 2. identities on resident fixtures ----------------------------------------------------------

def _linear():
    t = G.trace("sveltecomponent")
    return Doc(dt_amd.oplog_from_trace(t["txns"]).encode()), t["endContent"]


def test_identities_on_resident_fixtures():
    ff = Doc(G.dt_bytes("friendsforever"))
    lin, lin_end = _linear()
    ends = [G.trace("friendsforever_flat")["endContent"], lin_end]
    docs = [ff, lin]
    d = _resident(docs)
    req = []
    for k, x in enumerate(docs):
        tip, n = x.host.local_frontier(), len(x.host)
        req += [(k, [], tip), (k, tip, tip), (k, tip, [n // 2]), (k, [n // 2], [n // 3]), (k, [n // 2], tip)]
    m = d.xf_operations_from([r[0] for r in req], [r[1] for r in req], [r[2] for r in req])
    for k, x in enumerate(docs):
        tip = x.host.local_frontier()
        i = 5 * k
        # ROOT -> tip: the whole stream, the golden text
        assert _check(m, i, x, [], tip) == x.host.xf_operations_lv()
        assert m.content_bytes(i).decode() == ends[k]
        # tip -> tip: nothing to do
        assert _check(m, i + 1, x, tip, tip) == [] and m.version(i + 1) == tip
        assert m.content_bytes(i + 1).decode() == ends[k]
        # merging inside Hist(from): no records
        assert _check(m, i + 2, x, tip, req[i + 2][2]) == [] and m.version(i + 2) == tip
        if x.host.dominators(req[i + 3][1], req[i + 3][2]) == req[i + 3][1]:
            assert _check(m, i + 3, x, req[i + 3][1], req[i + 3][2]) == []
        else:
            _check(m, i + 3, x, req[i + 3][1], req[i + 3][2])
        _check(m, i + 4, x, req[i + 4][1], tip)
    # the linear trace: one entry, n // 3 is inside Hist(n // 2)
    assert m.xf_operations_lv(8) == []


# ---- 3. random requests against the oracle, four documents in one call ---------------------------

def _pairs(o, rng, k):
    n = len(o)
    out = []
    for _ in range(k):
        a = o.dominators(sorted(rng.sample(range(n), rng.choice([1, 1, 2]))))
        b = o.dominators(sorted(rng.sample(range(n), rng.choice([1, 1, 2]))))
        out.append((a, b))
    return out


def test_random_requests_four_documents_one_call():
    docs = [Doc(G.dt_bytes("friendsforever")), Doc(G.dt_bytes("git-makefile")),
            Doc(dt_amd.synth_oplog(0, 2000).encode()), Doc(dt_amd.synth_oplog(1, 2000).encode())]
    rng = random.Random(17)
    req = [(0, a, b) for a, b in _pairs(docs[0].host, rng, 6)]
    req += [(1, a, b) for a, b in _pairs(docs[1].host, rng, 2)]
    for k in (2, 3):
        n = len(docs[k].host)
        req.append((k, [n // 3], [2 * n // 3]))
    rng.shuffle(req)
    d = _resident(docs)
    m = d.xf_operations_from([r[0] for r in req], [r[1] for r in req], [r[2] for r in req])
    for i, (k, a, b) in enumerate(req):
        _check(m, i, docs[k], a, b)
    assert m.last_ms > 0 and len(m.profile(0)) == 8


# ---- 4. width limits -------------------------------------------------------------------------------

def test_width_limits_63_64_and_65():
    fans = {w: Doc(W.fan(w, merge=True).encode()) for w in (63, 64, 65)}
    order = [63, 65, 64]
    req = []
    for k, w in enumerate(order):
        x = fans[w]
        tips = W.branch_tips(x.host)
        assert len(tips) == w
        req.append((k, tips[1:], [tips[0]]))                   # the widest frontier less one tip, then that tip
        req.append((k, [tips[-1]], x.host.local_frontier()))   # one tip, then the merge tail
    d = _resident([fans[w] for w in order])
    m = d.xf_operations_from([r[0] for r in req], [r[1] for r in req], [r[2] for r in req])
    for i, (k, a, b) in enumerate(req):
        if order[k] == 65:
            assert m.status(i) == DEFER, (i, m.status(i))
            with pytest.raises(dt_amd.ParseError) as e:
                m.xf_operations_lv(i)
            assert e.value.code == DEFER
        else:
            _check(m, i, fans[order[k]], a, b, oracle=False)


# ---- 5. bad requests inside a good batch -----------------------------------------------------------

def test_bad_requests_leave_their_neighbours_alone():
    small = Doc(M.small_bytes())
    ff = Doc(G.dt_bytes("friendsforever"))
    bad = bytearray(small.data)
    bad[-1] ^= 0xFF   # the checksum
    bad = bytes(bad)
    with pytest.raises(dt_amd.ParseError) as e:
        dt_amd.ListOpLog.load_from(bad)
    want_bad = e.value.code
    d = dt_amd.DecodeBatch([small.data, bad, ff.data])
    d.run()
    n, nf = len(small.host), len(ff.host)
    tip = small.host.local_frontier()
    good = [(0, [3], tip), (2, [nf // 2], ff.host.local_frontier()), (0, [], [7])]
    req = [good[0], (0, [n], tip), (1, [3], [7]), good[1], (0, [], []), (0, [2], [n]), good[2], (2, [], [nf])]
    m = d.xf_operations_from([r[0] for r in req], [r[1] for r in req], [r[2] for r in req])
    assert [m.status(i) for i in range(len(req))] == [0, ERR_ARG, want_bad, 0, 0, ERR_ARG, 0, ERR_ARG]
    for i in (1, 2, 5, 7):   # a failed request has no frontier, no records and no text
        assert m._result(i)[1] == []
        for call in (m.xf_operations_lv, m.content_bytes, m.version):
            with pytest.raises(dt_amd.ParseError):
                call(i)
    # ROOT -> ROOT
    assert m.version(4) == [] and m.xf_operations_lv(4) == [] and m.content_bytes(4) == b""
    # the neighbours: what the same requests answer in a call of their own
    alone = d.xf_operations_from([g[0] for g in good], [g[1] for g in good], [g[2] for g in good])
    for j, i in enumerate((0, 3, 6)):
        k, a, b = good[j]
        got = _check(m, i, small if k == 0 else ff, a, b)
        assert got == alone.xf_operations_lv(j) and m.content_bytes(i) == alone.content_bytes(j)
        assert m.version(i) == alone.version(j)


# ---- 6. DecodeBatch.merge ------------------------------------------------------------------------------

def test_merge_four_branches_on_four_resident_copies():
    """The chain of test_gpu_branch_merge_applies_transformed_ops, four branches at once: after
    every step each branch's content is the oracle's checkout at its version; the last step reaches
    the golden text."""
    ff = Doc(G.dt_bytes("friendsforever"))
    d = _resident([ff] * 4)
    n = len(ff.host)
    rngs = [random.Random(29 + k) for k in range(4)]
    brs = [dt_amd.ListBranch.new() for _ in range(4)]
    for _ in range(5):
        d.merge(range(4), brs, [[r.randrange(n)] for r in rngs])
        for br in brs:
            assert br.content_bytes() == ff.text_at(br.local_frontier())
    d.merge(range(4), brs, [ff.host.local_frontier()] * 4)
    end = G.trace("friendsforever_flat")["endContent"]
    for br in brs:
        assert br.content() == end and br.local_frontier() == ff.host.local_frontier()


def _unicode_doc():
    o = dt_amd.ListOpLog()
    a, b = o.get_or_create_agent_id("ann"), o.get_or_create_agent_id("bo")
    o.add_insert_at(a, [], 0, "héllo wörld")
    o.add_insert_at(b, [4], 2, "ẑ日本")
    o.add_delete_at(a, [10], 1, 4)
    o.add_insert_at(a, [len(o) - 1], 0, "çà")
    o.add_delete_at(b, [13], 0, 2)
    o.add_insert_at(a, o.local_frontier(), 3, "fin…")
    return Doc(o.encode())


def test_merge_batch_iter_xf_operations_and_a_failed_branch():
    uni = _unicode_doc()
    ff = Doc(G.dt_bytes("friendsforever"))
    d = _resident([uni, ff])
    nu, nf = len(uni.host), len(ff.host)
    req = [(0, [], uni.host.local_frontier()), (0, [5], uni.host.local_frontier()), (1, [nf // 2], [nf - 1])]
    m = d.xf_operations_from([r[0] for r in req], [r[1] for r in req], [r[2] for r in req])
    for i, (k, a, b) in enumerate(req):
        x = uni if k == 0 else ff
        _check(m, i, x, a, b)
        assert list(m.iter_xf_operations(i)) == list(x.host.iter_xf_operations(a, b)), i
    assert any(op and op[0] == "ins" and any(ord(c) > 0x7F for c in op[2]) for _r, op in m.iter_xf_operations(0))
    # a branch whose request failed stays as it was; the others are updated before the error
    b0 = dt_amd.ListBranch.new_at_local_version(uni.host, [5])
    b1 = dt_amd.ListBranch.new_at_local_version(uni.host, [3])
    keep = (b0.content_bytes(), b0.local_frontier())
    with pytest.raises(dt_amd.ParseError) as e:
        d.merge([0, 0], [b0, b1], [[nu], uni.host.local_frontier()])
    assert e.value.code == ERR_ARG
    assert (b0.content_bytes(), b0.local_frontier()) == keep
    assert b1.local_frontier() == uni.host.local_frontier() and b1.content_bytes() == uni.ora.checkout_tip_bytes()


# ---- 7. after add: the server's sequence -----------------------------------------------------------------

def test_merge_after_add_from_the_old_frontier_to_the_new():
    """Resident documents held at a prefix version are patched to the tip (DecodeBatch.add), then
    merged from the old frontier to the new one on the merged batch.  The merged document numbers
    its LVs as part-then-patch, not as the full file does, so the records are checked against the
    host path over the same part and patch (load the part, decode_and_add the patch) and only the
    merged text against the full file's."""
    full = dt_amd.ListOpLog.load_from(G.dt_bytes("friendsforever"))
    end = G.trace("friendsforever_flat")["endContent"]
    n = len(full)
    parts, patches, hosts, olds = [], [], [], []
    for v in ([n // 2], [n // 3, 2 * n // 3], [n - 50]):
        f = full.dominators(v)
        part, patch = full.history(f).encode(), full.encode_from(f, dt_amd.ENCODE_PATCH)
        h = dt_amd.ListOpLog.load_from(part)
        olds.append(h.local_frontier())
        h.decode_and_add(patch)
        parts.append(part), patches.append(patch), hosts.append(h)
    d = dt_amd.DecodeBatch(parts)
    d.run()
    merged = d.add(patches)
    assert all(merged.add_result(i)[0] == 0 for i in range(3))
    m = merged.xf_operations_from(range(3), olds, [h.local_frontier() for h in hosts])
    for i, h in enumerate(hosts):
        assert m.status(i) == 0
        assert m.version(i) == h.local_frontier()
        assert m.xf_operations_lv(i) == h.xf_operations_lv(olds[i], h.local_frontier()), i
        assert m.content_bytes(i).decode() == end


def test_a_from_set_past_the_bound_is_deferred_alone():
    """`from` is reduced on one wave: more than 256 distinct LVs is DECODE_DEFER; 256 (and any
    number of repeats) is served, and the neighbour is not touched."""
    ff = Doc(G.dt_bytes("friendsforever"))
    d = _resident([ff])
    tip = ff.host.local_frontier()
    wide, most = list(range(100, 357)), list(range(100, 356)) * 2
    m = d.xf_operations_from([0, 0, 0], [wide, most, [355]], [tip, tip, tip])
    assert [m.status(i) for i in range(3)] == [DEFER, 0, 0]
    assert m._result(0)[1] == []
    _check(m, 1, ff, most, tip)
    _check(m, 2, ff, [355], tip)
