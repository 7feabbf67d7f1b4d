"""The designed compressor inputs of lz4_texts.py on the CPU: the host compressor's parse of each text
shows the property the text is named for, so test_gpu_lz4_compress.py provably drives the device
compressor into those corners.  Three properties of every host block hold independently of the
parse: the C oracle decompresses it to the input, the last sequence is literals only (at least
five bytes when the block has a match), and no match starts within the last 12 bytes or reaches
into the last 5."""
import pytest

import lz4_texts as T
from test_encoder import _oracle_lz4_decompress
import dt_amd


@pytest.mark.parametrize("name", list(T.texts()))
def test_text_reaches_its_corner(name):
    text, pred = T.texts()[name]
    raw = text.encode()
    assert raw.decode() == text
    block = dt_amd.lz4_compress(raw)
    seqs = T.parse_block(block)
    assert pred(seqs), seqs[:6]
    assert _oracle_lz4_decompress(block, len(raw)) == raw
    assert seqs[-1][1] == 0 and all(off for _, off, _ in seqs[:-1])
    at = 0
    for ll, off, ml in seqs[:-1]:
        at += ll
        assert at <= len(raw) - 12 and at + ml <= len(raw) - 5, (at, ml)
        at += ml
    if len(seqs) > 1:
        assert seqs[-1][0] >= 5


def test_backward_extension_past_64_bytes():
    """The parse is one literal run up to c and a match starting exactly at c.  The miss loop's
    probes over that run are the closed-form schedule (nothing matched before), and none of them
    falls into [c, c + 64): the match was found at least 64 bytes past c and extended backwards
    over all of them, which takes the extension loop's second round."""
    text, c, d = T.back_ext_text()
    assert T.parse(text) == [(c, d, d), (30, 0, 0)]
    probes = T.miss_probes(c + d)
    assert probes[0] == 1 and not any(c <= p < c + 64 for p in probes)
    found = min(p for p in probes if p >= c)
    assert found - c == T.BACK_EXT_STEP - 1 and found - d in probes


def test_named_parses():
    """The parses the far-offset, table and tail designs rest on, spelled out."""
    tx = T.texts()
    P = lambda n: T.parse(tx[n][0])
    assert P("far_65534")[1] == (0, 65534, 32) and P("far_65535")[1] == (0, 65535, 32)
    assert len(P("far_65536")) == 2   # the filler's one match, then literals: the marker is out of reach
    assert len(tx["far_u16"][0]) == 65534 and P("far_u16")[1] == (0, 65489, 32)
    assert [len(tx[f"table_{n}"][0].encode()) for n in T.TABLE_SIZES] == list(T.TABLE_SIZES)
    # the u16 and the u32 table hash differently: the parse changes between 65,534 and 65,535 bytes
    assert P("table_65534")[:200] != P("table_65535")[:200]
    assert [P(f"tail_{k}")[-1][0] for k in range(14)] == [6] * 7 + list(range(7, 14))
    for k in T.LIT_RUNS:
        assert P(f"lit_run_{k}")[1][0] == k
    for m in T.MATCH_LENS:
        assert P(f"ml_{m}")[0][2] == m
    # the output ring: some block crosses 512 and 1,024 compressed bytes inside an extension run
    crossed = set()
    for name in [n for n in tx if n.startswith("ring_")]:
        block, at = dt_amd.lz4_compress(tx[name][0].encode()), 0
        for ll, off, ml in T.parse_block(block):
            runs = [(at + 1, (ll - 15) // 255 + 1)] if ll >= 15 else []
            at += 1 + (runs[0][1] if runs else 0) + ll + (2 if off else 0)
            if off and ml >= 19:
                runs.append((at, (ml - 19) // 255 + 1))
                at += runs[-1][1]
            for start, n in runs:
                crossed |= {w for w in (512, 1024, 1536) if start < w < start + n}
    assert crossed == {512, 1024, 1536}
