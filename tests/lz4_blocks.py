"""Hand-built LZ4 raw blocks for the decoder tests: blocks the project's own compressor never
writes (chosen length extensions, offsets, sequence counts, token positions, no tail token),
malformed ones, and seeded random ones, each wrapped in a `.dt` file.

`build` writes a block from (literals, offset, match length) sequences and computes the plain
text by doing the copies itself, byte by byte: that is the reference for valid blocks, independent
of every decoder in the tree.  Literals are printable ASCII, so chars equal bytes and any copy is
valid UTF-8.  Host decoder and C oracle judge the invalid and random blocks (test_lz4_blocks.py
asserts that they agree); the device decoder is then compared with the host
(test_gpu_lz4_blocks.py).
"""
import functools
import random
import struct

import dt_amd
from dt_encode import chunk, crc32c, leb

_ALPHA = bytes(range(33, 127))


def lits(rng, n):
    return bytes(rng.choice(_ALPHA) for _ in range(n))


def _ext(v):
    out = bytearray()
    while v >= 255:
        out.append(255)
        v -= 255
    out.append(v)
    return bytes(out)


def seq_bytes(lit, off, ml):
    """One sequence as the format writes it; no check on off or ml beyond ml >= 4."""
    ll = len(lit)
    out = bytearray([(min(ll, 15) << 4) | min(ml - 4, 15)])
    if ll >= 15:
        out += _ext(ll - 15)
    out += lit
    out += struct.pack("<H", off)
    if ml - 4 >= 15:
        out += _ext(ml - 19)
    return bytes(out)


def tail_bytes(lit):
    ll = len(lit)
    out = bytearray([min(ll, 15) << 4])
    if ll >= 15:
        out += _ext(ll - 15)
    return bytes(out + lit)


def build(seqs, tail=b""):
    """(block, plain) of the sequences (literal bytes, offset, match length) and the final literals
    `tail`; tail=None writes no tail token at all: the block ends right after the last match."""
    block, plain = bytearray(), bytearray()
    for lit, off, ml in seqs:
        block += seq_bytes(lit, off, ml)
        plain += lit
        assert 1 <= off <= len(plain) and off < 65536 and ml >= 4, (off, ml, len(plain))
        for _ in range(ml):
            plain.append(plain[-off])
    if tail is not None:
        block += tail_bytes(tail)
        plain += tail
    else:
        assert seqs
    return bytes(block), bytes(plain)


def parse_block(block):
    """[(literal length, offset, match length)]; the tail, if any, is (literal length, 0, 0)."""
    out, ip, n = [], 0, len(block)
    while ip < n:
        tok = block[ip]
        ip += 1
        ll = tok >> 4
        if ll == 15:
            while True:
                b = block[ip]
                ip += 1
                ll += b
                if b != 255:
                    break
        ip += ll
        assert ip <= n
        if ip == n:
            out.append((ll, 0, 0))
            break
        off = block[ip] | (block[ip + 1] << 8)
        ip += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = block[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
        out.append((ll, off, ml + 4))
    return out


def _rd_leb(b, i):
    v = s = 0
    while True:
        x = b[i]
        i += 1
        v |= (x & 0x7F) << s
        s += 7
        if x < 0x80:
            return v, i


def swap_block(doc, block, ulen):
    """`doc` (first chunk CompressedFieldsLZ4) with that chunk's body replaced by leb(ulen) + block,
    the rest kept and the trailing CRC chunk rewritten."""
    assert doc[:8] == b"DMNDTYPS"
    _, i = _rd_leb(doc, 8)
    t, j = _rd_leb(doc, i)
    n, j = _rd_leb(doc, j)
    assert t == 5, "no CompressedFieldsLZ4 chunk (a text under 20 bytes is not compressed)"
    assert doc[-6] == 100 and doc[-5] == 4
    out = doc[:i] + chunk(5, leb(ulen) + bytes(block)) + doc[j + n:-6]
    return out + chunk(100, struct.pack("<I", crc32c(out)))


def doc_for(plain, runs=1):
    """One agent typing `plain` at the end in `runs` pieces, ENCODE_FULL: the file's LZ4 buffer is
    exactly the text."""
    text = plain.decode()
    assert len(plain) >= 20
    o = dt_amd.ListOpLog()
    a = o.get_or_create_agent_id("lz")
    step = -(-len(text) // runs)
    for i in range(0, len(text), step):
        o.add_insert(a, i, text[i:i + step])
    return o.encode(dt_amd.ENCODE_FULL)


def dt_of(block, plain, runs=1):
    return swap_block(doc_for(plain, runs), block, len(plain))


# ---- trains of short sequences ---------------------------------------------------------------
def train(rng, n, first=None, ext=False):
    """n sequences.  The first has `first` literals (a random 1..3 when None); the rest have 0..3
    literals and matches of 4..8 bytes at random offsets; with ext every one of the rest carries
    one length-extension byte (0 and 254 included), on the literals, the match or both."""
    seqs, op = [], 0
    for k in range(n):
        if k == 0 and first:
            ll = first
        else:
            ll = rng.randint(0 if op else 1, 3)
        ml = rng.randint(4, 8)
        if ext and (k or not first):
            which = rng.randrange(3)
            if which != 1:
                ll = 15 + rng.choice([0, 0, 1, 2, 5, 9, 30, 254] if rng.random() < 0.3 else [0, 1, 2, 3])
            if which != 0:
                ml = 19 + rng.choice([0, 0, 1, 2, 7, 40, 254] if rng.random() < 0.3 else [0, 1, 2, 3])
        op += ll
        r = rng.random()
        off = rng.randint(1, min(op, 4)) if r < 0.2 else rng.randint(1, min(op, 300)) if r < 0.8 else rng.randint(1, min(op, 65535))
        seqs.append((lits(rng, ll), off, ml))
        op += ml
    return seqs


def _out_len(seqs):
    return sum(len(l) + ml for l, _, ml in seqs)


# ---- part 2: directed valid blocks -----------------------------------------------------------
BIG_OUTPUT = 60000   # cases past this go with the batches that hold long blocks


@functools.lru_cache(maxsize=None)
def valid_cases():
    """{name: (block, plain)}."""
    rng = random.Random(20240)
    L = lambda n: lits(rng, n)
    T = lambda: L(3)   # a tail under the 5 literal bytes every compressor output ends with
    c = {}

    def add(name, seqs, tail=b"\0"):
        assert name not in c
        c[name] = build(seqs, T() if tail == b"\0" else tail)

    # length extensions
    for n in (0, 1, 14, 15, 16, 269, 270, 271, 524, 525, 526):
        add(f"lit_{n}", [(L(40), 7, 5), (L(n), 3, 6)])
        if n:
            add(f"lit_first_{n}", [(L(n), 1 + n // 2, 4), (b"", 1, 16)])
            add(f"lit_tail_{n}", [(L(21), 20, 4), (b"", 24, 4)], L(n))
    for m in (4, 18, 19, 20, 273, 274, 275, 528, 529):
        add(f"ml_{m}", [(L(600), 600, m)])
        add(f"ml_{m}_periodic", [(L(30), 3, m), (L(2), 2, m)])
    for k1, k2 in ((0, 0), (1, 254), (254, 1), (254, 254), (255, 255), (300, 300), (510, 509)):
        add(f"tok_ff_{k1}_{k2}", [(L(20), 5, 4), (L(15 + k1), 11, 19 + k2), (L(1), 1, 4)])
    # window phase: the train's tokens, offsets and extension bytes at every window offset
    for p in range(272):
        add(f"phase_{p}", train(rng, 80, first=p))
        add(f"phase_ext_{p}", train(rng, 40, first=p, ext=True))
    # batch boundaries
    for n in (63, 64, 65, 127, 128, 129):
        seqs = train(rng, n)
        add(f"train_{n}", seqs)
        add(f"train_{n}_empty_tail", seqs, b"")
        add(f"train_{n}_no_tail", seqs, None)
        add(f"train_{n}_tail_300", seqs, L(300))
        seqs = train(rng, n, ext=True)
        add(f"train_ext_{n}", seqs)
        add(f"train_ext_{n}_no_tail", seqs, None)
    # batch output size: the start map (at most 4,096 bytes) against the bisection
    for size in (4095, 4096, 4097):
        for lead in (0, 64):
            seqs = train(rng, lead) if lead else []
            base = _out_len(seqs)
            seqs.append((L(40), 9, 20))
            for _ in range(62):
                seqs.append((L(2), rng.randint(1, 60), 62))
            seqs.append((L(3), rng.randint(1, 3000), size - 62 * 64 - 60 - 3))
            assert _out_len(seqs) - base == size and len(seqs) == lead + 64
            add(f"batch_{size}_lead_{lead}", seqs)
    add("match_5000_periodic", [(L(100), 37, 5000)])
    add("match_5000", [(L(6000), 6000, 5000)])
    add("match_5000_second_batch", train(rng, 64) + [(L(1), 300, 5000)])
    add("match_70000", [(L(100), 100, 70000)])
    add("match_70000_off_1", [(L(70), 10, 10), (b"", 1, 70000)], None)
    # offsets
    for o in (1, 2, 3, 4):
        add(f"off_{o}", [(L(10), o, 40), (L(1), o, 5)])
    for ml in (4, 8, 33, 64, 65, 100):
        for d in (-1, 0, 1):
            add(f"off_ml_{ml}_{d:+d}", [(L(ml + 20), ml + d, ml)])
            add(f"off_ml_{ml}_{d:+d}_zero_lit", [(L(ml + 20), 7, 4), (b"", ml + d, ml)])
    add("off_whole_output", [(L(10), 10, 7), (L(5), 22, 9), (b"", 31, 40)])
    seqs = train(rng, 130)
    b1 = _out_len(seqs[:64])
    for k in range(12):   # one and two batches back
        op = _out_len(seqs) + 1
        seqs.append((L(1), op - (k if k % 2 else b1 + k), 4 + k))
    add("off_batches_back", seqs)
    for o in (1023, 1024, 1025):   # the edge of lz4_kernel's 1,024-entry ring, inside one batch
        add(f"off_ring_{o}", [(L(1500), o, 200), (L(1), o, 70)])
        add(f"off_ring_{o}_chain", [(L(1500), 900, 300), (b"", o, 200), (b"", o, 130)])
    for o in (65534, 65535):
        add(f"off_{o}", [(L(66000), o, 100), (L(2), o, 19)])
    # hop chains: every link copies from inside the previous one
    for links in (63, 64, 130):
        add(f"chain_{links}", [(L(20), 10, 8)] + [(b"", 8, 8)] * links)
        add(f"chain_{links}_periodic", [(L(20), 10, 8)] + [(b"", 5, 8)] * links)
        add(f"chain_{links}_mixed", [(L(9), 4, 9)] + [(b"", rng.randint(1, 9), 9) for _ in range(links)], None)
    add("zero_lit_run", [(L(25), 13, 6)] + [(b"", rng.randint(1, 30), rng.choice([4, 5, 18, 19, 20, 40])) for _ in range(20)])
    for name, (block, plain) in c.items():
        assert len(plain) >= 20, name
    return c


def is_big(plain):
    return len(plain) > BIG_OUTPUT


# ---- part 3: directed invalid blocks -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def invalid_cases():
    """{name: (block, claimed ulen, a plain text for the rest of the file)}.  Each fault is placed at
    sequence 0, at sequences 63 and 64 (the batch edge) and in a sequence whose lengths take two
    extension bytes (the exact parser's)."""
    rng = random.Random(4711)
    L = lambda n: lits(rng, n)
    c = {}
    ctxs = {"seq0": ([], 8, 6), "seq63": (train(rng, 63), 2, 6), "seq64": (train(rng, 64), 2, 6),
            "long_lit": (train(rng, 5), 300, 6), "long_ml": (train(rng, 5), 2, 300),
            "long_both": (train(rng, 70), 280, 290)}
    for cn, (pre, ll, ml) in ctxs.items():
        pb, pp = build(pre, None) if pre else (b"", b"")
        op = len(pp)
        good_block, good = build(pre + [(L(ll), 1, ml)], L(3))
        ref = good if len(good) >= 20 else good + L(20)

        def add(name, block, ulen, _cn=cn, _ref=ref):
            c[f"{name}_{_cn}"] = (bytes(block), ulen, _ref)

        lit = L(ll)
        add("offset_0", pb + seq_bytes(lit, 0, ml) + tail_bytes(L(3)), op + ll + ml + 3)
        add("offset_past_start", pb + seq_bytes(lit, op + ll + 1, ml) + tail_bytes(L(3)), op + ll + ml + 3)
        add("match_overruns_ulen", pb + seq_bytes(lit, 1, ml), op + ll + ml - 1)
        add("match_overruns_ulen_tail", pb + seq_bytes(lit, 1, ml) + tail_bytes(L(3)), op + ll + ml - 1)
        add("lit_overruns_ulen", pb + tail_bytes(lit), op + ll - 1)
        add("lit_overruns_ulen_seq", pb + seq_bytes(lit, 1, ml) + tail_bytes(L(3)), op + ll - 1)
        add("lit_overruns_input", (pb + tail_bytes(lit))[:-1], op + ll)
        add("lit_overruns_input_far", pb + tail_bytes(lit)[:1 + (ll >= 15) + (ll >= 270)], op + ll)
        add("ulen_minus_1", good_block, len(good) - 1)
        add("ulen_plus_1", good_block, len(good) + 1)
        add("ulen_huge", good_block, 255 * len(good_block) + 65)
        add("ulen_at_cap", good_block, 255 * len(good_block) + 64)
        # cuts inside a length extension (both lengths) and after one offset byte
        big = seq_bytes(L(15 + 255 + 7), 1, 19 + 255 + 7)
        add("cut_lit_ext_1", pb + big[:2], op + 300)
        add("cut_lit_ext_2", pb + big[:1], op + 300)
        add("cut_ml_ext", pb + big[:-1], op + 600)
        add("cut_ml_ext_2", pb + big[:-2], op + 600)
        s = seq_bytes(lit, 1, ml)
        cut = 1 + (ll >= 15) + (ll >= 270) + ll + 1
        add("cut_offset", pb + s[:cut], op + ll)
        add("cut_offset_0", pb + s[:cut - 1] + b"\0", op + ll)
    c["zero_lit_first"] = (seq_bytes(b"", 1, 4) + tail_bytes(L(20)), 24, L(24))
    c["zero_lit_first_long"] = (seq_bytes(b"", 1, 300) + tail_bytes(L(20)), 320, L(320))
    c["empty_block"] = (b"", 24, L(24))
    c["only_zero_token"] = (b"\0", 24, L(24))
    return c


# ---- part 3: seeded random blocks and their mutations ------------------------------------------
_LITS = [0, 0, 0, 1, 1, 2, 3, 14, 15, 16]
_LITS_LONG = [269, 270, 271, 524, 525, 526]
_MLS = [4, 4, 5, 6, 8, 18, 19, 20]
_MLS_LONG = [273, 274, 275, 528, 529]


def random_block(rng):
    n = int(round(400 ** rng.random()))   # 1 .. 400 sequences
    seqs, op = [], 0
    for _ in range(n):
        ll = rng.choice(_LITS_LONG) if rng.random() < 0.03 else rng.choice(_LITS)
        if op + ll == 0:
            ll = rng.choice([1, 14, 15, 16, 270])
        ml = rng.choice(_MLS_LONG) if rng.random() < 0.03 else rng.choice(_MLS)
        op += ll
        if rng.random() < 0.2:
            off = rng.randint(1, min(op, 65535))
        else:
            off = rng.choice([o for o in (1, 2, 3, 4, ml - 1, ml, ml + 1, op, op - 1) if 1 <= o <= min(op, 65535)])
        seqs.append((lits(rng, ll), off, ml))
        op += ml
    tail = [b"", None, lits(rng, rng.choice(_LITS)), lits(rng, rng.choice(_LITS_LONG))][rng.randrange(4)]
    return build(seqs, tail)


@functools.lru_cache(maxsize=None)
def random_cases(n_blocks=60, n_mut=20):
    """([(block, plain)], [(block, ulen, plain for the rest of the file)]): seeded valid blocks, and
    single-byte mutations of each (the claimed length stays)."""
    rng = random.Random(987)
    valid, mutated = [], []
    while len(valid) < n_blocks:
        block, plain = random_block(rng)
        if len(plain) < 20:
            continue
        valid.append((block, plain))
        for _ in range(n_mut):
            b = bytearray(block)
            k = rng.randrange(len(b))
            b[k] = rng.choice([0, 255, b[k] ^ 0x10, b[k] ^ 0x01, b[k] ^ 0xF0, rng.randrange(256)])
            if bytes(b) != block:
                mutated.append((bytes(b), len(plain), plain))
    return valid, mutated


@functools.lru_cache(maxsize=None)
def valid_docs():
    """[(name, .dt bytes, plain)] of the directed and the random valid blocks; the text is typed in
    one, two or three runs."""
    out = []
    for k, (name, (block, plain)) in enumerate(valid_cases().items()):
        out.append((name, dt_of(block, plain, runs=1 + k % 3), plain))
    for k, (block, plain) in enumerate(random_cases()[0]):
        out.append((f"random_{k}", dt_of(block, plain), plain))
    return out


@functools.lru_cache(maxsize=None)
def invalid_docs():
    """[(name, .dt bytes)] of the directed invalid blocks."""
    return [(name, swap_block(doc_for(ref), block, ulen)) for name, (block, ulen, ref) in invalid_cases().items()]


@functools.lru_cache(maxsize=None)
def mutated_docs():
    """[.dt bytes] of the random mutations.  One file per base block is built and its block swapped,
    so the text after the block is encoded once."""
    out, base = [], {}
    for block, ulen, plain in random_cases()[1]:
        if plain not in base:
            base[plain] = doc_for(plain)
        out.append(swap_block(base[plain], block, ulen))
    return out
