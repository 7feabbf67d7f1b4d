"""Every device entry point at the 64-lane widths: frontiers, versions, parent lists, causal chains
and retreat / advance passes of exactly 63, 64 and 65 (the fans of wide_docs.py; their structure
is pinned on the CPU by test_wide_docs.py).

The rule of every case: up to 64 the device answers with status 0 and the exact result -- the host
code's arrays and bytes, the oracle's text, the plain models of wide_docs.py; past 64 a path whose
documented limit is 64 (DECODE_MAX_FRONTIER, DECODE_MAX_PARENTS, PREP_MAX_CHAINS) answers with
exactly DECODE_DEFER, or with the base document's own status where the base was deferred: never a
wrong result, never another status, and the deferred set is asserted to be exactly the items past
64.  Every wide item sits between ordinary neighbours in the same call -- a 1-fan and
friendsforever, for requests a one-LV request on each side -- and the neighbours' arrays,
frontiers and texts are asserted as well: the per-document version and frontier slots are exactly
64 words, so one element too many lands in the neighbour's slot, whose owner still reports 0.
The errors the neighbours are there to catch are of this kind: `fn >= DECODE_MAX_FRONTIER` relaxed
to `fn > DECODE_MAX_FRONTIER` where the decoder appends to the frontier (dt_decode.hip,
decode_doc's frontier advance), or the `fi < DECODE_MAX_FRONTIER` guard dropped from the history
mark's frontier write (dt_mark.hpp, mark_doc)."""
import random

import numpy as np
import pytest

import golden_data as G
import wide_docs as W
from oracle.oracle import OpLog as OracleOpLog
from test_gpu_decode import WHAT
from test_gpu_history import _dev_exact, _host_exact
from test_gpu_parity import _host_plan, _same_plan
from test_gpu_patch import OPTION_SETS, _host_patch
from test_gpu_replay_short_paths import BIG_OPS, _tiers
import dt_amd

pytestmark = pytest.mark.gpu

DEFER = dt_amd.DECODE_DEFER
LIMIT = 64   # DECODE_MAX_FRONTIER = DECODE_MAX_PARENTS = PREP_MAX_CHAINS
SINGLE = [("del_same",), ("del_same2",), ("ins_same",)]
ENCODER_OPTS = [dt_amd.ENCODE_FULL, dt_amd.EncodeOptions(True, False, True), dt_amd.EncodeOptions(False, True, True)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if dt_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the engine has no CPU fallback")


@pytest.fixture(scope="module")
def nb():
    """The ordinary neighbours: a 1-fan and friendsforever, as bytes, host oplogs and texts."""
    one, ff = W.fan(1).encode(), G.dt_bytes("friendsforever")
    texts = {one: OracleOpLog.load_from(one).checkout_tip_bytes(),
             ff: G.trace("friendsforever_flat")["endContent"].encode()}
    return one, ff, {one: dt_amd.ListOpLog.load_from(one), ff: dt_amd.ListOpLog.load_from(ff)}, texts


def _between(wide, one, ff):
    """The wide items with an ordinary neighbour on each side (the 1-fan and friendsforever in
    turn): (documents, index of each wide item)."""
    docs, at = [], []
    for k, d in enumerate(wide):
        docs.append(ff if k % 2 else one)
        at.append(len(docs))
        docs.append(d)
    docs.append(ff if len(wide) % 2 else one)
    return docs, at


def _arrays_equal(dec, i, host):
    for w in WHAT:
        a, b = dec.export(i, w), host.export(w)
        if w == "agent_names":
            assert a == b, (i, w)
        else:
            assert np.array_equal(a, b), (i, w, a[:8], b[:8])
    assert dec.status(i)["n_lv"] == len(host)


def _applied(part, patches):
    host = dt_amd.ListOpLog.load_from(part)
    for p in patches:
        host.decode_and_add(p)
    return host


def _oracle_at(host, front):
    """The oracle's text of `host` at `front`, for documents whose LV order no file keeps (they
    arrived as parts): the host's history sub-oplog (pinned by test_checkout_version.py) as a file."""
    return OracleOpLog.load_from(host.history(front).encode()).checkout_tip_bytes()


# ---- decode -----------------------------------------------------------------------------------------
def test_decode(nb):
    """DecodeBatch.run over the unmerged and merged fans of every width and an as_parts base: every
    array (version included) equals ListOpLog.load_from, the neighbours' too; exactly the fans past
    64 are deferred.  Widths 8 / 9 straddle the batched history path's np <= 8 (wider parent lists
    take the exact path); no profile slot tells the two apart, so only the arrays are compared."""
    one, ff, hosts, _ = nb
    wide = [(w, W.fan(w, merge=m).encode()) for w in W.WIDTHS for m in (False, True)]
    wide.append((0, W.as_parts(8)[1]))
    docs, at = _between([d for _, d in wide], one, ff)
    dec = dt_amd.DecodeBatch(docs)
    dec.run()
    width_at = {i: w for i, (w, _) in zip(at, wide)}
    deferred = [i for i in range(len(docs)) if dec.status(i)["status"] == DEFER]
    assert [width_at.get(i) for i in deferred] == [w for w, _ in wide if w > LIMIT]
    for i, d in enumerate(docs):
        if i in deferred:
            continue
        assert dec.status(i)["status"] == 0, (i, width_at.get(i), dec.status(i))
        _arrays_equal(dec, i, hosts[d] if d in hosts else dt_amd.ListOpLog.load_from(d))


# ---- decode_and_add ---------------------------------------------------------------------------------
def test_add_at_the_frontier_and_start_branch_limits(nb):
    """A 60-wide frontier grown by 3, 4 and 5 concurrent branches (63 and 64 merge, 65 is deferred
    and the resident document is as it was); the W-parent merge as a patch on bases of 63, 64 and
    65 branches (its StartBranch version is W wide; the 65-fan base was deferred itself, and that
    status is the answer)."""
    one, ff, _, _ = nb
    cases = [W.grown(60, e)[1:] for e in (3, 4, 5)] + [W.grown(b, 0, merge=True)[1:] for b in (63, 64, 65)]
    want = [0, 0, DEFER, 0, 0, DEFER]
    bases, at = _between([b for b, _ in cases], one, ff)
    patches, _ = _between([p for _, p in cases], one, ff)   # the neighbours add themselves (all overlap)
    d = dt_amd.DecodeBatch(bases)
    d.run()
    base_want = {at[5]: DEFER}
    assert [d.status(i)["status"] for i in range(len(bases))] == [base_want.get(i, 0) for i in range(len(bases))]
    m = d.add(patches)
    want_at = dict(zip(at, want))
    for i, (b, p) in enumerate(zip(bases, patches)):
        st, f = m.add_result(i)
        assert st == want_at.get(i, 0), (i, st)
        if i in base_want:
            assert m.status(i)["status"] == DEFER
            continue
        host = dt_amd.ListOpLog.load_from(b)
        if st == 0:
            assert sorted(f) == sorted(host.decode_and_add(p)), i
        assert m.status(i)["status"] == 0
        assert _dev_exact(m, i) == _host_exact(host), i
    assert len(m.export(at[1], "version")) == 64 and len(m.export(at[2], "version")) == 60


def test_add_link_by_link():
    """The interleaved as_parts documents built through add(), one link at a time as
    test_gpu_patch.test_walk_order does: 63 and 64 branches, 8 at a time, between 8-fans that grow
    beside them; every link equals the host's oplog after the same decode_and_add.  The 65th
    branch's first patch is deferred and leaves its document, and the neighbours, as they were."""
    widths = [8, 63, 8, 64, 8, 65, 8]
    chains = [W.as_parts(w, k=1 if w == 8 else 8) for w in widths]
    links = 24
    assert [len(c[2]) for c in chains] == [24, 24, 24, 24, 24, 27, 24]
    hosts = [dt_amd.ListOpLog.load_from(c[1]) for c in chains]
    cur = dt_amd.DecodeBatch([c[1] for c in chains])
    cur.run()
    for k in range(links):
        cur = cur.add([c[2][k] for c in chains])
        for i, c in enumerate(chains):
            st, f = cur.add_result(i)
            hf = hosts[i].decode_and_add(c[2][k])
            assert st == 0 and sorted(f) == sorted(hf), (i, k, st)
            assert _dev_exact(cur, i) == _host_exact(hosts[i]), (i, k)
    for i in (1, 3):   # LV order kept: the oplog as it was built
        for what in ("entries", "parents", "parent_offsets", "ops", "version"):
            assert _host_exact(hosts[i])[what] == _host_exact(chains[i][0])[what], (i, what)
    assert len(cur.export(3, "version")) == 64 and len(cur.export(5, "version")) == 64
    last = cur.add([c[2][links if i == 5 else links - 1] for i, c in enumerate(chains)])
    for i, c in enumerate(chains):
        st, _f = last.add_result(i)
        assert st == (DEFER if i == 5 else 0), (i, st)
        if i != 5:
            hosts[i].decode_and_add(c[2][links - 1])
        assert last.status(i)["status"] == 0
        assert _dev_exact(last, i) == _host_exact(hosts[i]), i
    b = last.checkout_batch()
    b.run()
    b.sync()
    res = b.results()
    for i, w in enumerate(widths):
        assert res[i]["status"] == 0, (i, res[i])
        assert b.text(i) == OracleOpLog.load_from(W.fan(min(w, 64)).encode()).checkout_tip_bytes(), i


# ---- history, encode_from, checkout at a version ----------------------------------------------------
@pytest.fixture(scope="module")
def resident(nb):
    """One resident handle: [1-fan, 64-fan, friendsforever, merged 66-fan (deferred at decode),
    1-fan, the 66-wide halves document (held: its frontier never passes 34), 1-fan] -- the halves
    document arrives as a part and a patch, so the handle is a decode_and_add result -- with the
    host oplogs and the requests: (document, version, status), each wide one between one-LV ones."""
    one, ff, hosts, _ = nb
    f64 = W.fan(64).encode()
    f66 = W.fan(66, merge=True).encode()
    _, hpart, hpatch = W.halves(66)
    bases = [one, f64, ff, f66, one, hpart, one]
    d = dt_amd.DecodeBatch(bases)
    d.run()
    assert [d.status(i)["status"] for i in range(7)] == [0, 0, 0, DEFER, 0, 0, 0]
    m = d.add([one, f64, ff, f66, one, hpatch, one])
    assert [m.add_result(i)[0] for i in range(7)] == [0, 0, 0, DEFER, 0, 0, 0]
    h64, h66, hh = dt_amd.ListOpLog.load_from(f64), dt_amd.ListOpLog.load_from(f66), _applied(hpart, [hpatch])
    ho = {0: hosts[one], 1: h64, 2: hosts[ff], 3: h66, 4: hosts[one], 5: hh, 6: hosts[one]}
    for i in (0, 1, 2, 4, 5, 6):
        assert _dev_exact(m, i) == _host_exact(ho[i]), i
    t64, t66, th = h64.local_frontier(), W.branch_tips(h66), W.branch_tips(hh)
    assert (len(t64), len(t66), len(th)) == (64, 66, 66) and max(th) > 127
    rng = random.Random(64)

    def shuffled(v, repeats):
        v = list(v) + rng.sample(list(v), repeats)
        rng.shuffle(v)
        return v

    every_lv_of_64 = list(range(len(h64)))                      # unreduced: reduces to the 64 tips
    assert h64.dominators(every_lv_of_64) == t64
    lvs_of_64_branches = [x for x in range(len(hh)) if hh.dominators([x] + th[:64]) == th[:64]]
    assert hh.dominators(lvs_of_64_branches) == th[:64] and len(lvs_of_64_branches) == 10 + 5 * 64
    wide = [
        (1, t64[:63], 0), (1, t64, 0), (1, every_lv_of_64, 0), (1, shuffled(t64, 9), 0),
        (3, t66[:64], DEFER), (3, t66[:65], DEFER),             # the base's own status
        (5, th[:63], 0), (5, th[:64], 0), (5, lvs_of_64_branches, 0), (5, shuffled(th[:64], 7), 0),
        (5, shuffled(th[1:64], 5), 0),
        (5, th[:65], DEFER), (5, th, DEFER), (5, shuffled(th[:65], 11), DEFER), (5, th[1:], DEFER),
    ]
    # the request after a wide one is on a 1-fan: the least work, so it is written first and a
    # neighbour's overrun lands on top of it
    small = [(0, [3]), (4, [12]), (6, [14]), (2, [100])]
    reqs = [(2, [20000], 0)]
    for k, r in enumerate(wide):
        reqs.append(r)
        d_, v = small[k % 3] if r[2] else small[k % 4]
        reqs.append((d_, v, 0))
    return m, ho, reqs


def test_history_and_its_checkout(resident):
    """Requests 63, 64 and 65 wide (in order, unreduced, shuffled with repeats) in one history
    call: status 0 up to 64 with the host's dominators and every array of host.history(v), exactly
    DECODE_DEFER past 64; then the handle's device checkout against the oracle."""
    m, ho, reqs = resident
    h = m.history([d for d, _, _ in reqs], [v for _, v, _ in reqs])
    fronts = []
    for i, (d, v, want) in enumerate(reqs):
        st, f = h.history_result(i)
        assert st == want, (i, d, len(v), st)
        fronts.append(f)
        if want:
            assert h.status(i)["status"] == want, i
            continue
        assert h.status(i)["status"] == 0, i
        assert f == ho[d].dominators(v), (i, d)
        assert _dev_exact(h, i) == _host_exact(ho[d].history(v)), (i, d, len(v))
    assert sorted({len(f) for f, r in zip(fronts, reqs) if not r[2]}) == [1, 63, 64]
    b = h.checkout_batch()
    b.run()
    b.sync()
    res = b.results()
    for i, (d, v, want) in enumerate(reqs):
        assert res[i]["status"] == want, (i, res[i])
        if not want:
            assert b.text(i) == _oracle_at(ho[d], fronts[i]), (i, d, len(v))
    # where a file keeps the LV order the oracle reads the version itself
    ora = OracleOpLog.load_from(W.fan(64).encode())
    assert b.text(1) == ora.checkout_bytes(fronts[1]) and b.text(3) == ora.checkout_bytes(fronts[3])


@pytest.mark.parametrize("opts", OPTION_SETS, ids=["patch", "uncompressed", "no_content"])
def test_encode_from(resident, opts):
    """The same requests as patches: byte for byte the host encoder's.  A 64-wide request is the
    full Version stream (PATCH_FRONT_BYTES; the halves document's tips lie above LV 127)."""
    m, ho, reqs = resident
    pb = m.encode_from([d for d, _, _ in reqs], [v for _, v, _ in reqs], opts)
    for i, (d, v, want) in enumerate(reqs):
        assert pb.status(i) == want, (i, d, len(v), pb.status(i))
        if want:
            with pytest.raises(dt_amd.ParseError) as e:
                pb.patch(i)
            assert e.value.code == want
            continue
        assert pb.frontier(i) == ho[d].dominators(v), (i, d)
        assert pb.patch(i) == _host_patch(ho[d], v, opts), (i, d, len(v))


def test_checkout_versions(resident):
    """63- and 64-wide versions check out to host.checkout(v) and the oracle's text; a 65-wide one,
    and any version of the merged 66-fan the decoder deferred, raise DECODE_DEFER."""
    m, ho, _ = resident
    th, t66 = W.branch_tips(ho[5]), W.branch_tips(ho[3])
    docs, vs = [0, 5, 4, 5, 6, 1, 0], [[3], th[:63], [12], th[2:66], [14], ho[1].local_frontier()[1:], [9]]
    got = m.checkout_versions(docs, vs)
    for d, v, br in zip(docs, vs, got):
        want = ho[d].checkout(v)
        assert br.content_bytes() == want.content_bytes() == _oracle_at(ho[d], sorted(v)), (d, len(v))
        assert br.local_frontier() == want.local_frontier() == sorted(v), (d, len(v))
    for d, v in ((5, th[:65]), (5, th), (3, t66[:63]), (3, t66[:64]), (3, t66[:65])):
        with pytest.raises(dt_amd.ParseError) as e:
            m.checkout_versions([0, d, 4], [[3], v, [12]])
        assert e.value.code == DEFER, (d, len(v))


def test_the_loop_on_the_device(nb):
    """history -> encode_from -> add -> checkout on a 64-fan and a merged 64-fan: the history at 63
    tips plus its patch is 64 wide again, and the patch from the 64 tips of the merged fan is the
    64-parent merge under a 64-wide StartBranch version."""
    one, ff, hosts, texts = nb
    f64, m64 = W.fan(64).encode(), W.fan(64, merge=True).encode()
    docs = [one, f64, ff, m64, one]
    h64, hm = dt_amd.ListOpLog.load_from(f64), dt_amd.ListOpLog.load_from(m64)
    want = [texts[one], OracleOpLog.load_from(f64).checkout_tip_bytes(), texts[ff],
            OracleOpLog.load_from(m64).checkout_tip_bytes(), texts[one]]
    base = dt_amd.DecodeBatch(docs)
    base.run()
    t64, tm = h64.local_frontier(), W.branch_tips(hm)
    assert len(tm) == 64 and hm.dominators(tm) == tm
    idx = [0, 1, 2, 3, 4, 1, 0, 3, 4]
    vs = [[3], t64[:63], [1000], tm, [7], t64[32:], [9], tm[:63], [14]]
    hist = base.history(idx, vs)
    pb = base.encode_from(idx, vs)
    assert [pb.status(i) for i in range(len(idx))] == [0] * len(idx)
    assert [pb.frontier(i) for i in range(len(idx))] == [hist.history_result(i)[1] for i in range(len(idx))] == vs
    m = hist.add([pb.patch(i) for i in range(len(idx))])
    assert [m.add_result(i)[0] for i in range(len(idx))] == [0] * len(idx)
    ho = [hosts[one], h64, hosts[ff], hm, hosts[one]]
    for k, i in enumerate(idx):   # the host's own loop is the checker of the merged arrays
        sub = ho[i].history(vs[k])
        sub.decode_and_add(_host_patch(ho[i], vs[k], dt_amd.ENCODE_PATCH))
        assert _dev_exact(m, k) == _host_exact(sub), k
    b = m.checkout_batch()
    b.run()
    b.sync()
    res = b.results()
    for k, i in enumerate(idx):
        assert res[k]["status"] == 0, (k, res[k])
        assert b.text(k) == want[i], k


# ---- checkout ---------------------------------------------------------------------------------------
def test_checkout_device_staged(nb):
    """Device-staged checkout of the mixed fans of every width (15 / 16 / 17 straddle chain_kernel's
    16 chains, 63 / 64 / 65 prep's 64) and of the single-op shapes at 63-66: the oracle's text, the
    plain model's for the single-op shapes, the device plan equal to the host plan and nothing
    planned on the host up to 64 chains; the documents past 64 chains are exactly the deferred
    set, and the host-staged retry checks them out."""
    one, ff, hosts, texts = nb
    wide = [(w, None, W.fan(w, merge=m).encode()) for w in W.WIDTHS for m in (False, True)]
    wide += [(w, s, W.fan(w, s).encode()) for s in SINGLE for w in (63, 64, 65, 66)]
    docs, at = _between([d for _, _, d in wide], one, ff)
    want = {i: OracleOpLog.load_from(d).checkout_tip_bytes() for i, (_, _, d) in zip(at, wide)}
    for i, (w, s, _) in zip(at, wide):
        if s is not None:
            assert want[i].decode() == W.model_text(w, s), (w, s)
    b = dt_amd.Batch(docs=docs, staging="device")
    b.run()
    b.sync()
    res = b.results()
    width_at = {i: w for i, (w, _, _) in zip(at, wide)}
    deferred = [i for i in range(len(docs)) if res[i]["status"] == DEFER]
    assert [width_at.get(i) for i in deferred] == [w for w, _, _ in wide if w > LIMIT]
    planned, linear = b.host_planned(), b.fast_forwarded()
    # (a 1-fan is a linear history: it checks out on the fast-forward path, which has no walk plan)
    assert [i for i in range(len(docs)) if linear[i]] == [i for i, d in enumerate(docs) if d == one or width_at.get(i) == 1]
    for i, d in enumerate(docs):
        if i in deferred:
            continue
        assert res[i]["status"] == 0, (i, width_at.get(i), res[i])
        assert b.text(i) == (want[i] if i in want else texts[d]), (i, width_at.get(i))
        assert planned[i] == 0, (i, width_at.get(i))
        if i in want and not linear[i]:
            _same_plan(b.plan(i), _host_plan(dt_amd.ListOpLog.load_from(d)))
    retry, rat = _between([docs[i] for i in deferred], one, ff)
    h = dt_amd.Batch(docs=retry, staging="host")
    h.run()
    h.sync()
    res = h.results()
    assert [r["status"] for r in res] == [0] * len(retry)
    for k, i in zip(rat, deferred):
        assert h.text(k) == want[i], width_at[i]
    for k, d in enumerate(retry):
        if k not in rat:
            assert h.text(k) == texts[d], k


@pytest.fixture(scope="module")
def host_staged(nb):
    """Oplogs for the host-staged batches, for the short base and for one that outgrows the smallest
    LDS index (8 blocks): test_gpu_replay_short_paths.BIG_OPS = 3,000 LVs hand back to the HBM tier
    there, and a base that long does here (3,000 characters are 94 blocks):
    per width 65, 66 and 96 the merged mixed fan, interleaved as built (an entry per step), and the
    single-op shapes -- all-delete passes of 64, 65 and 95 entries on one item, and as many sibling
    inserts at one position -- between a 1-fan and friendsforever.  {base_len: (oplogs, texts, wide)}"""
    one, ff, hosts, texts = nb
    out = {}
    for base_len in (10, BIG_OPS):
        wide = []
        for w in (65, 66, 96):
            wide.append((w, None, W.fan(w, merge=True, base_len=base_len, interleave=True)))
            wide += [(w, s, W.fan(w, s, base_len=base_len)) for s in SINGLE]
        oplogs, want, is_wide = [], [], []
        for k, (w, s, o) in enumerate(wide):
            oplogs.append(hosts[ff] if k % 2 else hosts[one])
            want.append(texts[ff] if k % 2 else texts[one])
            oplogs.append(o)
            t = OracleOpLog.load_from(o.encode()).checkout_tip_bytes()
            if s is not None:
                assert t.decode() == W.model_text(w, s, base_len), (w, s)
            want.append(t)
            is_wide += [False, True]
        oplogs.append(hosts[one])
        want.append(texts[one])
        is_wide.append(False)
        out[base_len] = (oplogs, want, is_wide)
    return out


@pytest.mark.parametrize("env,base_len,flags,tier", [
    ({}, 10, 0, 1), ({"DTGPU_FLAT": "0"}, 10, 0, 1), ({"DTGPU_DEBUG": "1"}, 10, 0, 1),
    ({"DTGPU_LDS_FILL": "4000"}, BIG_OPS, dt_amd.OPT_NO_SEGMENTS, 0)], ids=["flat", "lds3", "debug", "hbm_handback"])
def test_checkout_host_staged(monkeypatch, host_staged, env, base_len, flags, tier):
    """The fans past 64 chains, which only the host-staged path replays: the 64- and 65-entry
    single-item delete passes and 64 and more same-position siblings on the flat LDS tier, the
    3-level LDS tier, the instrumented kernel and (with a base long enough) the HBM tier.  (There
    friendsforever replays uncut: the LDS index is sized for the largest document or segment of the
    tier, and its segments' placeholders would size it past the fans.)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    oplogs, want, is_wide = host_staged[base_len]
    b = dt_amd.Batch(oplogs=oplogs, flags=flags)
    b.run()
    b.sync()
    res = b.results()
    assert [r["status"] for r in res] == [0] * len(oplogs), [(i, r) for i, r in enumerate(res) if r["status"]]
    for i in range(len(oplogs)):
        assert b.text(i) == want[i], i
        if is_wide[i]:
            assert _tiers(b, i) == {tier}, (i, _tiers(b, i))


# ---- the batched encoder ----------------------------------------------------------------------------
@pytest.mark.parametrize("opts", ENCODER_OPTS, ids=["full", "uncompressed", "no_content"])
def test_batch_encode(nb, opts):
    """Batch.encode over the fans up to 64: byte for byte the host encoder's (test_gpu_encode.py's
    option sets)."""
    one, ff, hosts, _ = nb
    wide = [W.fan(w, merge=m).encode() for w in W.WIDTHS if w <= LIMIT for m in (False, True)]
    docs, _ = _between(wide, one, ff)
    b = dt_amd.Batch(docs=docs, staging="device")
    b.encode(opts)
    for i, d in enumerate(docs):
        assert b.encoded_status(i) == 0, i
        assert b.encoded(i) == (hosts[d] if d in hosts else dt_amd.ListOpLog.load_from(d)).encode(opts), i
