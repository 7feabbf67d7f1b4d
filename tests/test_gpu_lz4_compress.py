"""The device LZ4 compressor (enc::Lz::run, csrc/dt_enc_dev.hpp) on the designed texts of
lz4_texts.py, whose host parses test_lz4_texts.py pins to the corners they are named for: the
table switch at 65,535 bytes, offsets up to 65,535, literal runs around the 64 that emit_lits
holds in registers, extension runs longer than 64 bytes, tails around the last-12 and last-5
limits, steps whose probes share hashes, a candidate at position 0, extension runs across the
output ring's wrap, and multi-byte text.

Every file the device writes equals the host encoder's byte for byte, in each instantiation of
the compressor: the ROOT encoder reading its text from HBM, the same with the text staged in LDS
(DTGPU_ENC_LDS_TEXT), and the patch encoder (encode_from, dt_patch.hip)."""
import pytest

import lz4_texts as T
import dt_amd

pytestmark = pytest.mark.gpu

LDS_TEXT = 24064


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if dt_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the engine has no CPU fallback")


@pytest.fixture(scope="module")
def corpus():
    """(names, .dt files, the host encoder's bytes for each): built once."""
    names = list(T.texts())
    docs = [T.doc_of(T.texts()[n][0]) for n in names]
    host = [dt_amd.ListOpLog.load_from(d).encode() for d in docs]
    return names, docs, host


@pytest.mark.parametrize("lds_text", [None, str(LDS_TEXT)], ids=["hbm_text", "lds_text"])
def test_device_compressor_equals_host(monkeypatch, corpus, lds_text):
    names, docs, host = corpus
    if lds_text:
        monkeypatch.setenv("DTGPU_ENC_LDS_TEXT", lds_text)
        sizes = [len(T.texts()[n][0].encode()) for n in names]
        assert min(sizes) <= LDS_TEXT < max(sizes)   # both instantiations in the one batch
    b = dt_amd.Batch(docs=docs, staging="device")
    b.encode()
    for i, n in enumerate(names):
        assert b.encoded_status(i) == 0, n
        assert b.encoded(i) == host[i], n


def test_device_compressor_counters(monkeypatch, corpus):
    """With the encoder's profile on: the bytes are the same, the device found exactly the host
    parse's matches, and the small-alphabet texts went through steps whose probes share a hash."""
    names, docs, host = corpus
    monkeypatch.setenv("DTGPU_ENC_PROF", "1")
    b = dt_amd.Batch(docs=docs, staging="device")
    b.encode()
    for i, n in enumerate(names):
        assert b.encoded(i) == host[i], n
        prof = b.encode_profile(i)
        assert prof["lz_sequences"] == len(T.parse(T.texts()[n][0])) - 1, n
        if n.startswith("alphabet_"):
            assert prof["lz_shared_steps"] > 100, (n, prof)


def test_patch_encoder_compressor_equals_host(corpus):
    """encode_from from ROOT and from the first two LVs (the text without its first one or two
    characters): dt_patch.hip's instantiation against the host's encode_from."""
    names, docs, _ = corpus
    hosts = [dt_amd.ListOpLog.load_from(d) for d in docs]
    dec = dt_amd.DecodeBatch(docs)
    dec.run()
    for i in range(len(docs)):
        assert dec.status(i)["status"] == 0, names[i]
    idx = list(range(len(docs)))
    for req in ([], [0], [1]):
        pb = dec.encode_from(idx, [req] * len(docs), dt_amd.ENCODE_PATCH)
        for i, n in enumerate(names):
            assert pb.status(i) == 0, (n, req)
            assert pb.patch(i) == hosts[i].encode_from(req, dt_amd.ENCODE_PATCH), (n, req)
