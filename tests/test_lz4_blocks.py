"""The hand-built LZ4 blocks of lz4_blocks.py on the CPU: the host decoder and the C oracle accept
every valid block and give the text that lz4_blocks.build computed by doing the copies itself; on
the malformed and the mutated blocks the two return the same status.  That makes the host decoder
the judge of the device decoder in test_gpu_lz4_blocks.py.  None of the valid blocks is what the
project's own compressor writes for the same text, which is why they are here."""
import collections

import lz4_blocks as B
from oracle.oracle import OpLog as OracleOpLog, OracleError
from test_encoder import _lz4_chunk, _oracle_lz4_decompress
import dt_amd


def _host_code(data):
    try:
        dt_amd.ListOpLog.load_from(data)
        return 0
    except dt_amd.ParseError as e:
        return e.code


def _oracle_code(data):
    try:
        OracleOpLog.load_from(data)
        return 0
    except OracleError as e:
        return e.code


def test_builder_and_parser_round_trip():
    """build writes the format: a known block by hand, and parse_block inverts seq_bytes."""
    block, plain = B.build([(b"abcd", 4, 6), (b"", 1, 19)], b"xy")
    assert block == bytes([0x42]) + b"abcd" + bytes([4, 0, 0x0F, 1, 0, 0, 0x20]) + b"xy"
    assert plain == b"abcdabcdab" + b"b" * 19 + b"xy"
    assert B.parse_block(block) == [(4, 4, 6), (0, 1, 19), (2, 0, 0)]
    block, _ = B.build([(b"q" * 270, 3, 274)], None)
    assert block == bytes([0xFF, 255, 0]) + b"q" * 270 + bytes([3, 0, 255, 0])
    assert B.parse_block(block) == [(270, 3, 274)]
    for name, (block, plain) in B.valid_cases().items():
        seqs = B.parse_block(block)
        assert sum(ll + ml for ll, _, ml in seqs) == len(plain), name


def test_swap_block_keeps_the_file():
    """Swapping a file's own block back in returns the file, CRC included."""
    doc = B.doc_for(b"hello hello hello hello hello world", runs=2)
    ul, block = _lz4_chunk(doc)
    assert ul == 35 and B.swap_block(doc, block, ul) == doc


def test_directed_valid_blocks():
    docs = B.valid_docs()
    assert len(docs) > 700
    same = []
    for name, doc, plain in docs:
        ul, block = _lz4_chunk(doc)
        assert ul == len(plain), name
        assert _host_code(doc) == 0, name
        assert _oracle_code(doc) == 0, name
        assert bytes(dt_amd.ListOpLog.load_from(doc).export("content")) == plain, name
        assert _oracle_lz4_decompress(block, ul) == plain, name
        assert OracleOpLog.load_from(doc).checkout_tip_bytes() == plain, name
        if dt_amd.lz4_compress(plain) == block:
            same.append(name)
    # (a random block of one or two sequences can be what the greedy parse finds too)
    assert [n for n in same if not n.startswith("random_")] == [] and len(same) <= 3, same


def test_directed_cases_cover_what_they_name():
    """The shapes the cases are named for, read back from the blocks."""
    c = B.valid_cases()
    P = lambda name: B.parse_block(c[name][0])
    for n in (0, 1, 14, 15, 16, 269, 270, 271, 524, 525, 526):
        assert P(f"lit_{n}")[1][0] == n
    for m in (4, 18, 19, 20, 273, 274, 275, 528, 529):
        assert P(f"ml_{m}")[0][2] == m
    assert c["lit_270"][0][44:47] == bytes([0xF2, 255, 0])          # the extension ends with a 0 byte
    assert c["ml_274"][0][-6:-4] == bytes([255, 0])
    for n in (63, 64, 65, 127, 128, 129):
        assert len(P(f"train_{n}_no_tail")) == n and P(f"train_{n}_no_tail")[-1][1] != 0
        assert P(f"train_{n}_empty_tail")[-1] == (0, 0, 0) and c[f"train_{n}_empty_tail"][0][-1] == 0
        assert P(f"train_{n}_tail_300")[-1] == (300, 0, 0)
    for size in (4095, 4096, 4097):
        s = P(f"batch_{size}_lead_0")
        assert len(s) == 65 and sum(ll + ml for ll, _, ml in s[:64]) == size
    assert max(ml for _, _, ml in P("match_70000")) == 70000
    assert [o for _, o, _ in P("off_65535")][:2] == [65535, 65535]
    assert [s[1:] for s in P("chain_64")[1:65]] == [(8, 8)] * 64
    # every window offset 0..255 holds a token in some case of the sweep, extension bytes too
    tok_at, ext_at = set(), set()
    for name, doc, plain in B.valid_docs():
        if not name.startswith("phase_"):
            continue
        ul, block = _lz4_chunk(doc)
        at = doc.index(block)
        ip = 0
        for ll, off, ml in B.parse_block(block):
            tok_at.add((at + ip) % 256)
            ip += 1
            if ll >= 15:
                ext_at.add((at + ip) % 256)
                ip += 1 + (ll - 15) // 255
            ip += ll
            if off:
                ip += 2
                if ml >= 19:
                    ext_at.add((at + ip) % 256)
                    ip += 1 + (ml - 19) // 255
    assert len(tok_at) == 256 and len(ext_at) == 256


def test_invalid_and_mutated_blocks_host_equals_oracle():
    """Every malformed and every mutated block: the host decoder's status is the oracle's.  The
    directed faults are all refused; the mutations are a mix of accepted and refused."""
    for name, doc in B.invalid_docs():
        h = _host_code(doc)
        assert h == _oracle_code(doc), name
        assert h != 0, name
    seen = collections.Counter()
    for i, doc in enumerate(B.mutated_docs()):
        h = _host_code(doc)
        assert h == _oracle_code(doc), i
        seen[h] += 1
    assert len(B.mutated_docs()) > 1000
    # 7: LZ4DecompressionError; 13: InvalidUTF8 (a mutated literal or a copy from another place)
    assert seen[0] > 100 and seen[7] > 100 and seen[13] > 100, seen
