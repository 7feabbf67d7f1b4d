"""Designed inputs for the LZ4 compressor tests: texts that steer the greedy parse (lz4_flex's, restated
in csrc/dt_encode.cpp and replayed lane-parallel by enc::Lz::run in csrc/dt_enc_dev.hpp) into its
corners.  Every text comes with a predicate on the host compressor's parse, which
test_lz4_texts.py asserts, so each input provably reaches the corner it is named for; where the
parse depends on parity effects of the miss loop, the builder searches seeds until the parse shows
the property.  All texts are valid UTF-8 (ASCII unless named otherwise).
"""
import functools
import random

import dt_amd
from lz4_blocks import parse_block

_ALPHA = "".join(chr(c) for c in range(33, 127) if chr(c) not in "#!")


def rnd(rng, n, alpha=_ALPHA):
    return "".join(rng.choice(alpha) for _ in range(n))


def parse(text):
    """The host compressor's sequences for `text`: [(literal length, offset, match length)]."""
    return parse_block(dt_amd.lz4_compress(text.encode()))


def _search(make, pred, tries=400):
    """The first make(seed) whose host parse satisfies pred."""
    for seed in range(tries):
        t = make(seed)
        if pred(parse(t)):
            return t
    raise AssertionError("no seed gives the parse asked for")


def has_seq(ll=None, off=None, ml=None, first=0):
    return lambda seqs: any((ll is None or s[0] == ll) and (off is None or s[1] == off) and
                            (ml is None or s[2] == ml) and s[1] for s in seqs[first:])


def far_text(d, seed=1):
    """A 32-byte marker, a 0123456789 filler (one giant match, so the miss counter is fresh at the
    second marker), the marker again at distance d, then ! and a random tail."""
    rng = random.Random(seed)
    marker = rnd(rng, 32)
    filler = ("0123456789" * (d // 10 + 1))[:d - 32]
    return marker + filler + marker + "!" + rnd(rng, 40)


def miss_probes(limit):
    """The positions the miss loop probes from position 1 while nothing matches: a run of k misses
    steps by (32 + k) >> 5 bytes."""
    out, pos, nmc = [], 1, 32
    while pos < limit:
        out.append(pos)
        pos += nmc >> 5
        nmc += 1
    return out


BACK_EXT_STEP = 72   # the miss loop's step where back_ext_text puts its copy


def back_ext_text(seed=0):
    """(text, c, d): random text, and at c a copy of the d = 3 steps bytes before c.  c lies one byte
    past a probe of the miss loop, where the step is 72: no probe falls into the copy's first 64
    bytes, so the match is found 71 bytes into it and extended backwards over 71 bytes: more than
    one 64-lane round.  (A literal run has to pass 68 KB before the step passes 64.)"""
    rng = random.Random(seed)
    probes = miss_probes(200000)
    j = next(k for k in range(len(probes) - 1) if probes[k + 1] - probes[k] == BACK_EXT_STEP) + 8
    c, d = probes[j] + 1, 3 * BACK_EXT_STEP
    body = rnd(rng, c)
    return body + body[c - d:] + rnd(rng, 30), c, d


LIT_RUNS = (14, 15, 16, 63, 64, 65, 269, 270, 271)
MATCH_LENS = (18, 19, 20, 273, 274, 275)
TABLE_SIZES = (65533, 65534, 65535, 65536, 65537)
SMALL_SIZES = (20, 21, 24, 25, 32)


@functools.lru_cache(maxsize=None)
def texts():
    """{name: (text, predicate on the host parse)}."""
    t = {}
    # table choice: the u16 table below 65,535 bytes, the u32 table from there
    rng = random.Random(3)
    vocab = [rnd(rng, rng.randint(2, 9), "abcdefghijklmnop") for _ in range(300)]
    prose = " ".join(rng.choice(vocab) for _ in range(14000))
    for n in TABLE_SIZES:
        t[f"table_{n}"] = (prose[:n], lambda s: len(s) > 3000 and max(o for _, o, _ in s) > 60000)
    # far offsets: found at 65,534 and 65,535, out of reach at 65,536
    for d in (65534, 65535):
        t[f"far_{d}"] = (far_text(d), has_seq(off=d))
    t["far_65536"] = (far_text(65536), lambda s: not any(o >= 65000 for _, o, _ in s))
    # the largest offset the u16 table can yield: the text ends 13 bytes after the second marker
    def u16_far(seed):
        rng = random.Random(seed)
        marker = rnd(rng, 32)
        d = 65534 - 32 - 13
        return marker + ("0123456789" * 6600)[:d - 32] + marker + "!" + rnd(rng, 12)
    t["far_u16"] = (_search(u16_far, has_seq(off=65534 - 45)), has_seq(off=65534 - 45))
    assert len(t["far_u16"][0]) == 65534
    # literal runs before a match: emit_lits up to 64 pending literals, emit past that
    for k in LIT_RUNS:
        def lit_run(seed, k=k):
            rng = random.Random(seed)
            word = rnd(rng, 12 + seed % 5)
            return word + "#" + word + rnd(rng, k + (seed // 5) % 3 - 1) + word + rnd(rng, 30)
        t[f"lit_run_{k}"] = (_search(lit_run, has_seq(ll=k, first=1)), has_seq(ll=k, first=1))
    # extension runs of more than 64 bytes
    rng = random.Random(5)
    def lit_ext(seed):
        rng = random.Random(seed)
        word = rnd(rng, 80)
        return word + "#" + word + rnd(rng, 16336) + word + rnd(rng, 20)
    long_lits = lambda s: any(ll > 15 + 255 * 64 and off for ll, off, _ in s)
    t["lit_ext_run"] = (_search(lit_ext, long_lits), long_lits)
    t["ml_ext_run"] = (rnd(rng, 20) + "ab" * 9000 + rnd(rng, 20),
                       lambda s: any(ml > 19 + 255 * 64 for _, _, ml in s))
    t["ml_ext_run_far"] = (rnd(rng, 3000) * 7 + rnd(rng, 20), lambda s: any(ml > 19 + 255 * 64 and off == 3000 for _, off, ml in s))
    # a backward extension of more than 64 bytes
    text, c, d = back_ext_text()
    t["back_ext"] = (text, lambda s, c=c, d=d: s[0] == (c, d, d) and len(s) == 2)
    # match lengths around the one- and two-byte extensions
    for m in MATCH_LENS:
        def match_len(seed, m=m):
            rng = random.Random(seed)
            word = rnd(rng, m)
            return word + "#" + word + "!" + rnd(rng, 20)
        t[f"ml_{m}"] = (_search(match_len, has_seq(ml=m)), has_seq(ml=m))
    # tails: a match, then 0..13 more bytes; the last five bytes are always literals
    rng = random.Random(6)
    word = rnd(rng, 24)
    for k in range(14):
        tail = rnd(rng, k)
        want = 6 if k <= 6 else None
        t[f"tail_{k}"] = (word + "#" + word + tail,
                          lambda s, want=want, k=k: len(s) == 2 and s[0][1] == 25 and (s[1][0] == want if want else s[1][0] >= k))
    for n in SMALL_SIZES:
        t[f"small_{n}"] = (("abcdefg" * 5)[:n], lambda s, n=n: (len(s) == 2 and s[0][1] == 7 and s[0][0] + s[0][2] + s[1][0] == n)
                           if n > 20 else len(s) >= 1)
        t[f"small_periodic_{n}"] = ("x" * n, lambda s: len(s) == 2 and s[0][:2] == (1, 1))
    # shared hashes: few distinct 4-grams, so probes of one step collide
    for letters, n in (("ab", 30000), ("abc", 30000), ("ab", 100000), ("abc", 100000)):
        rng = random.Random(7 + n + len(letters))
        t[f"alphabet_{len(letters)}_{n}"] = (rnd(rng, n, letters),
                                             lambda s: len(s) > 3000 and max(ll for ll, _, _ in s) <= 40)
    # position 0: the first 4-gram recurs, so the candidate equals the table's zero entry
    rng = random.Random(8)
    head = rnd(rng, 9)
    t["position_0"] = (head + rnd(rng, 31) + head + rnd(rng, 30), has_seq(ll=40, off=40))
    head = rnd(rng, 100)
    t["position_0_late"] = (head + rnd(rng, 5000) + head + rnd(rng, 30), has_seq(off=5100))
    # the 512-byte output ring: a first sequence of about 500 compressed bytes, then a literal run
    # with five extension bytes, so that this extension run, the literal copy and the offset cross
    # the first wrap at every phase; and a literal run that puts a match's six extension bytes
    # across the second and the third wrap
    for k in range(0, 24):
        rng = random.Random(100 + k)
        w1 = rnd(rng, 16)
        text = w1 + rnd(rng, 470 + k) + w1 + rnd(rng, 1100) + "z" * 1300 + rnd(rng, 30)
        t[f"ring_{k}"] = (text, lambda s: any(ll >= 15 + 255 * 4 and off for ll, off, _ in s) and
                          any(ml >= 19 + 255 * 4 for _, _, ml in s))
        for wrap, a in ((1024, 1004), (1536, 1516)):
            t[f"ring_{wrap}_{k}"] = (rnd(rng, a + k) + "z" * 1300 + rnd(rng, 30),
                                     lambda s: len(s) == 2 and s[0][2] >= 19 + 255 * 4)
    # multi-byte characters: the parse works on bytes, a match may start inside a character
    rng = random.Random(9)
    parts = ["héllo", "wörld", "日本語", "テキスト", "😀", "𝄞", "plain", "ascii", "ß", "€"]
    t["multibyte"] = (" ".join(rng.choice(parts) for _ in range(3000)), lambda s: len(s) > 500)
    word = "é日😀" * 4
    t["multibyte_lit_run"] = (word + rnd(rng, 300) + "𝄞" + word + rnd(rng, 30), lambda s: any(off and ll > 64 for ll, off, _ in s))
    return t


def doc_of(text):
    """One agent typing `text` at the end: the encoder's LZ4 input is exactly the text."""
    o = dt_amd.ListOpLog()
    o.add_insert(o.get_or_create_agent_id("lz"), 0, text)
    return o.encode(dt_amd.ENCODE_FULL)
