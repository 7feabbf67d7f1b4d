"""The device LZ4 decompressor (lz4_block, dt_decode.hip) on blocks the project's compressor never
writes: the hand-built valid, malformed and mutated blocks of lz4_blocks.py, which
test_lz4_blocks.py pins to the C oracle through the host decoder.

Every block goes through each instantiation of lz4_block: one wave inside decode_kernel (the
default for short blocks, and DTGPU_NO_LZ_PRE for all), the three-wave lz4_kernel with its
resolved-source ring (DTGPU_LZ_PRE_MIN=1), the two-wave one (DTGPU_LZ3_MAX=0) and decode_and_add's.
A valid block decodes (never DECODE_DEFER) to the host decoder's arrays, and its content is the
text lz4_blocks.build computed; a directed malformed block gets exactly the host's status; of the
random mutations at most 1 in 20 may be handed back, the others equal the host."""
import pytest

import golden_data as G
import lz4_blocks as B
from test_gpu_decode import _host_code, _same_arrays
from test_gpu_decode_add import _check_batch
import dt_amd

pytestmark = pytest.mark.gpu

CONFIGS = {
    "one_wave_short": ({}, False),
    "three_waves": ({"DTGPU_LZ_PRE_MIN": "1"}, True),
    "two_waves": ({"DTGPU_LZ_PRE_MIN": "1", "DTGPU_LZ3_MAX": "0"}, True),
    "one_wave_all": ({"DTGPU_NO_LZ_PRE": "1"}, True),
}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if dt_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the engine has no CPU fallback")


@pytest.fixture(scope="module")
def host_codes():
    """The host decoder's status of every invalid and mutated file, computed once."""
    return ([_host_code(d) for _, d in B.invalid_docs()], [_host_code(d) for d in B.mutated_docs()])


def _neighbours():
    return [G.dt_bytes("friendsforever"), G.COMPAT_SIMPLE_LZ4]


def _valid(big):
    return [(n, d, p) for n, d, p in B.valid_docs() if big or not B.is_big(p)]


@pytest.mark.parametrize("config", list(CONFIGS))
def test_valid_blocks(monkeypatch, config):
    env, big = CONFIGS[config]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cases = _valid(big)
    assert big == any(B.is_big(p) for _, _, p in cases)
    docs, where = [], []
    for k, (name, d, plain) in enumerate(cases):
        if k % 100 == 0:
            docs += _neighbours()
        where.append(len(docs))
        docs.append(d)
    dec = dt_amd.DecodeBatch(docs)
    dec.run()
    for i, d in enumerate(docs):
        assert dec.status(i)["status"] == 0, i
    for (name, d, plain), i in zip(cases, where):
        assert bytes(dec.export(i, "content")) == plain, name
        _same_arrays(dec, i, d)
    for i in (0, 1):
        _same_arrays(dec, i, docs[i])


@pytest.mark.parametrize("config", list(CONFIGS))
def test_invalid_and_mutated_blocks(monkeypatch, config, host_codes):
    env, _ = CONFIGS[config]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    inv, mut = B.invalid_docs(), B.mutated_docs()
    # one batch: the directed faults between ordinary neighbours, then the mutations
    docs = _neighbours() + [d for _, d in inv] + _neighbours() + list(mut) + _neighbours()
    dec = dt_amd.DecodeBatch(docs)
    dec.run()
    for i in (0, 1, 2 + len(inv), 3 + len(inv), len(docs) - 2, len(docs) - 1):
        assert dec.status(i)["status"] == 0, i
        _same_arrays(dec, i, docs[i])
    for k, (name, d) in enumerate(inv):
        assert dec.status(2 + k)["status"] == host_codes[0][k], name
    deferred = 0
    for k, d in enumerate(mut):
        i = 4 + len(inv) + k
        got = dec.status(i)["status"]
        if got == dt_amd.DECODE_DEFER:
            deferred += 1
            continue
        assert got == host_codes[1][k], k
        if got == 0:
            _same_arrays(dec, i, d)
    assert deferred <= len(mut) // 20


def test_valid_blocks_as_patches_onto_an_empty_oplog():
    """decode_and_add's instantiation: every valid file merged into an empty oplog equals the host's
    merge, with status 0; the malformed ones are refused with the host's status and leave it empty."""
    cases = _valid(True)
    pairs = [(None, d) for _, d, _ in cases]
    pairs.insert(300, (None, G.COMPAT_SIMPLE_LZ4))
    pairs.append((None, G.dt_bytes("friendsforever")))
    m, sts = _check_batch(pairs)
    assert all(s == 0 for s in sts), [i for i, s in enumerate(sts) if s]
    assert bytes(m.export(0, "content")) == cases[0][2]
    assert bytes(m.export(len(pairs) - 2, "content")) == cases[-1][2]
    _, sts = _check_batch([(None, d) for _, d in B.invalid_docs()])
    assert all(s not in (0, dt_amd.DECODE_DEFER) for s in sts), sts


def test_valid_blocks_check_out_on_the_device():
    """One device-staged batch: every text is the one lz4_blocks.build computed."""
    cases = _valid(True)
    docs = [d for _, d, _ in cases] + _neighbours()
    b = dt_amd.Batch(docs=docs, staging="device")
    b.run()
    b.sync()
    res = b.results()
    for i, (name, d, plain) in enumerate(cases):
        assert res[i]["status"] == 0, name
        assert b.text(i) == plain, name
    assert res[-1]["status"] == 0 and b.text(len(docs) - 1) == G.COMPAT_SIMPLE_TEXT.encode()
    assert res[-2]["status"] == 0
