// dt_enc_dev.hpp -- device helpers of the `.dt` writers, shared by the ROOT encoder (dt_encoder.hip)
// and the patch encoder (dt_patch.hip): the wave-wide byte copy, varints (leb.rs), chunk ids, the
// lane-parallel CRC-32C, lz4_flex 0.10's greedy parse with 64 probe positions per step (see
// dt_encode.cpp lz4_block_compress) and write_op's varint head (encode_oplog.rs:20-92).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dt_wave.hpp"

namespace dtgpu {
namespace enc {
using namespace wave;

// wave-wide byte copy, eight loads in flight per lane before their stores
DEV void copy_bytes(uint8_t *dst, const uint8_t *src, uint32_t n) {
    uint32_t i = lane();
    for (; i + 7 * 64 < n; i += 8 * 64) {
        uint8_t v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = src[i + 64 * k];
#pragma unroll
        for (int k = 0; k < 8; k++) dst[i + 64 * k] = v[k];
    }
    for (; i < n; i += 64) dst[i] = src[i];
}

// ---- varints (leb.rs) ---------------------------------------------------------------------------
DEV uint32_t leb_len(uint64_t v) {
    uint32_t n = 1;
    while (v >= 0x80) { v >>= 7; n++; }
    return n;
}
DEV uint32_t put_leb(uint8_t *d, uint64_t v) {
    uint32_t n = 0;
    while (v >= 0x80) { d[n++] = uint8_t(v | 0x80); v >>= 7; }
    d[n++] = uint8_t(v);
    return n;
}
DEV uint64_t zz_old(int64_t v) { return (uint64_t(v < 0 ? -v : v) << 1) | (v < 0 ? 1u : 0u); }

constexpr uint32_t ST_OK = 0, ST_CHECKOUT = 64, ST_CAPACITY = 65;
constexpr uint32_t C_LZ4 = 5, C_FILEINFO = 1, C_DOCID = 2, C_AGENTNAMES = 3, C_STARTBRANCH = 10, C_CONTENT = 13,
                   C_CONTENTCOMP = 14, C_PATCHES = 20, C_OPVERSIONS = 21, C_OPTYPEPOS = 22, C_OPPARENTS = 23,
                   C_PATCHCONTENT = 24, C_CONTENTKNOWN = 25, C_CRC = 100;

// ---- CRC-32C (combine helpers: dt_wave.hpp) ------------------------------------------------------
// s must be 16-byte aligned: each lane's segment is a multiple of 16 bytes, read as uint4 words
// with the next word in flight while the current one goes through the table
DEV uint32_t crc_word(uint32_t c, uint32_t w, const uint32_t *T) {
    c ^= w;
    c = T[c & 0xFFu] ^ (c >> 8);
    c = T[c & 0xFFu] ^ (c >> 8);
    c = T[c & 0xFFu] ^ (c >> 8);
    return T[c & 0xFFu] ^ (c >> 8);
}
DEV uint32_t crc32c_par(const uint8_t *s, uint32_t n, const uint32_t *T, const uint32_t *x2n) {
    const uint32_t S = ((n + 63) / 64 + 15) & ~15u;
    const uint32_t b0 = lane() * S;
    const uint32_t e0 = b0 < n ? min(b0 + S, n) : b0;
    uint32_t c = ~0u;
    uint32_t i = b0;
    if (i + 16 <= e0) {
        const uint4 *w = reinterpret_cast<const uint4 *>(s + i);
        uint4 cur = w[0];
        for (uint32_t k = 1;; k++) {
            const bool more = i + 32 <= e0;
            const uint4 nxt = more ? w[k] : cur;
            c = crc_word(c, cur.x, T);
            c = crc_word(c, cur.y, T);
            c = crc_word(c, cur.z, T);
            c = crc_word(c, cur.w, T);
            i += 16;
            if (!more) break;
            cur = nxt;
        }
    }
    for (; i < e0; i++) c = T[(c ^ s[i]) & 0xFFu] ^ (c >> 8);
    c = ~c;
    if (e0 <= b0) c = 0;
    const uint32_t op_full = x2nmodp(x2n, S, 3);
    uint32_t crc = rdl(c, 0);
    for (uint32_t l = 1; l < 64; l++) {
        const uint32_t sb = l * S;
        if (sb >= n) break;
        const uint32_t len = sb + S <= n ? S : n - sb;
        crc = multmodp(len == S ? op_full : x2nmodp(x2n, len, 3), crc) ^ rdl(c, l);
    }
    return crc;
}

// ---- LZ4 (lz4_flex 0.10 compress_into, restated in dt_encode.cpp) -----------------------------
DEV uint32_t ld32(const uint8_t *p) {
    return uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24);
}
DEV uint64_t ld64(const uint8_t *p) { return uint64_t(ld32(p)) | (uint64_t(ld32(p + 4)) << 32); }

// sum_{i < x} (i >> 5): the miss loop's probe offsets in closed form (step = nmc >> 5, nmc += 1)
DEV uint64_t probe_sum(uint64_t x) {
    const uint64_t q = x >> 5, r = x & 31;
    return 16 * q * (q - (q ? 1 : 0)) + r * q;
}

typedef __attribute__((address_space(3))) uint16_t LDS16;
typedef __attribute__((address_space(3))) uint32_t LDS32;

constexpr uint32_t LZ_RING = 512;   // LDS staging of the compressed bytes (flushed to HBM)

struct Lz {
    const uint8_t *in;   // the text: LDS or HBM (one address space per instantiation site)
    uint8_t *out;        // HBM
    uint8_t *ring;       // LDS, LZ_RING bytes
    uint32_t n, o, f;    // text length, bytes emitted, bytes flushed
    bool small, prof;
    uint32_t st[4];      // profile: probe steps, steps with shared hashes, sequences, -
    uint64_t cyc[3];     // profile: cycles in probing, extending, emitting
    uint32_t *tab;   // LDS: 8,192 u16 (small) or 4,096 u32
    DEV uint32_t hash(uint32_t p) const {
        if (small) return (ld32(in + p) * 2654435761u) >> 19;
        return uint32_t(((ld64(in + p) << 24) * 889523592379ull) >> 52);
    }
    // volatile LDS (address space 3) accesses: ds ops that are never forwarded or merged
    DEV uint32_t vget(uint32_t h) const {
        return small ? uint32_t(((volatile LDS16 *)tab)[h]) : ((volatile LDS32 *)tab)[h];
    }
    DEV void vput(uint32_t h, uint32_t v) {
        if (small) ((volatile LDS16 *)tab)[h] = uint16_t(v);
        else ((volatile LDS32 *)tab)[h] = v;
    }
    // the output goes through the LDS ring, so the parse never waits on HBM stores (vmcnt)
    DEV void flush() {
        for (uint32_t i = f + lane(); i < o; i += 64) out[i] = ring[i & (LZ_RING - 1)];
        f = o;
    }
    DEV void reserve(uint32_t k) {   // k <= 128
        if (o + k - f > LZ_RING) flush();
    }
    DEV void put1(uint8_t v) {
        reserve(1);
        if (lane() == 0) ring[o & (LZ_RING - 1)] = v;
        o++;
    }
    DEV void ext(uint32_t v) {   // 255-run length extension
        const uint32_t nb = v / 255 + 1;
        for (uint32_t x = 0; x < nb; x += 64) {
            const uint32_t k = min(64u, nb - x);
            reserve(k);
            if (lane() < k) ring[(o + lane()) & (LZ_RING - 1)] = x + lane() + 1 < nb ? 255 : uint8_t(v - 255 * (nb - 1));
            o += k;
        }
    }
    // emit() with the (<= 64) literals already in registers: lane j holds in[l0 + j]
    DEV void emit_lits(uint32_t l0, uint32_t l1, uint32_t lb, uint32_t off, uint32_t mlen) {
        const uint32_t ll = l1 - l0;
        put1(uint8_t((min(ll, 15u) << 4) | min(mlen - 4, 15u)));
        if (ll >= 15) ext(ll - 15);
        reserve(ll);
        if (lane() < ll) ring[(o + lane()) & (LZ_RING - 1)] = uint8_t(lb);
        o += ll;
        put1(uint8_t(off));
        put1(uint8_t(off >> 8));
        if (mlen - 4 >= 15) ext(mlen - 19);
    }
    DEV void emit(uint32_t l0, uint32_t l1, uint32_t off, uint32_t mlen) {
        const uint32_t ll = l1 - l0;
        put1(uint8_t((min(ll, 15u) << 4) | (off ? min(mlen - 4, 15u) : 0u)));
        if (ll >= 15) ext(ll - 15);
        for (uint32_t x = 0; x < ll; x += 64) {
            const uint32_t k = min(64u, ll - x);
            reserve(k);
            if (lane() < k) ring[(o + lane()) & (LZ_RING - 1)] = in[l0 + x + lane()];
            o += k;
        }
        if (!off) return;
        put1(uint8_t(off));
        put1(uint8_t(off >> 8));
        if (mlen - 4 >= 15) ext(mlen - 19);
    }
    DEV uint32_t run() {
        o = f = 0;
        small = n < 65535;
        st[0] = st[1] = st[2] = st[3] = 0;
        cyc[0] = cyc[1] = cyc[2] = 0;
        uint64_t tc = prof ? clock64() : 0;
        auto tick = [&](int k) {
            if (prof) { const uint64_t t = clock64(); cyc[k] += t - tc; tc = t; }
        };
        for (uint32_t i = lane(); i < 4096; i += 64) tab[i] = 0;
        if (n < 13) { emit(0, n, 0, 0); flush(); return o; }
        const uint32_t end_check = n - 12, match_lim = n - 6;
        uint32_t lit = 0, cur = 1;   // position 0 is hashed first: its entry is the table's zero
        const uint32_t l = lane();
        for (;;) {
            uint32_t nmc = 32, pos = cur, cand = 0;
            bool found = false;
            // probes of the miss loop: 16 in the first step (a match is usually a few bytes
            // away: fewer shared hashes to resolve), 64 in later ones
            for (uint32_t width = 16;; width = 64) {
                const uint64_t base = probe_sum(nmc);
                const uint32_t p = pos + uint32_t(probe_sum(nmc + l) - base);
                const bool valid = l < width && p <= end_check;
                const uint32_t nv = popc(ballot(valid));   // valid probes form a prefix
                const uint32_t h = valid ? hash(p) : 0xFFFFFFFFu;
                const uint32_t w32 = valid ? ld32(in + p) : 0u;
                // every probe writes its position into its slot and reads the slot back: when
                // each probe won its own slot, no two probes share a hash and the table held
                // every candidate (volatile: the read-back must see the other lanes' writes)
                const uint32_t old = valid ? vget(h) : 0u;
                const uint32_t cw = valid ? ld32(in + old) : 0u;   // in flight across the slot check
                if (valid) vput(h, p);
                const bool won = !valid || vget(h) == p;
                uint32_t c, lim;
                uint64_t m;
                st[0]++;
                if (!ballot(!won)) {
                    c = old;
                    const bool ok = valid && p - c <= 65535u && cw == w32;
                    m = ballot(ok);
                    lim = m ? ctz(m) + 1 : nv;
                    if (valid && l >= lim) vput(h, old);   // probes past the match never ran
                } else {   // shared hashes: a probe's candidate is the last earlier probe of its hash
                    st[1]++;
                    if (valid) vput(h, old);
                    // one ballot per contested hash: each group lost at least one slot write
                    uint64_t lost = ballot(!won);
                    int prevj = -1;
                    uint32_t nextj = 64;
                    while (lost) {
                        const uint32_t hj = rdl(h, ctz(lost));
                        const bool mine = valid && h == hj;
                        const uint64_t g = ballot(mine);
                        if (mine) {
                            const uint64_t below = g & lt_mask(), above = g & ~lt_mask() & ~(1ull << l);
                            prevj = below ? int(63 - __clzll((long long)below)) : -1;
                            nextj = above ? ctz(above) : 64;
                        }
                        lost &= ~g;
                    }
                    const uint32_t pp = uint32_t(__shfl(int(p), prevj < 0 ? int(l) : prevj));
                    c = prevj >= 0 ? pp : old;
                    const bool ok = valid && p - c <= 65535u && (prevj >= 0 ? ld32(in + c) : cw) == w32;
                    m = ballot(ok);
                    lim = m ? ctz(m) + 1 : nv;
                    if (l < lim && nextj >= lim) vput(h, p);   // the last probe of each hash wins
                }
                if (m) {
                    cur = rdl(p, lim - 1);
                    cand = rdl(c, lim - 1);
                    found = true;
                    break;
                }
                if (nv < width) break;   // past len - 12: the tail is literals
                pos += uint32_t(probe_sum(nmc + width) - base);
                nmc += width;
            }
            tick(0);
            if (!found) { emit(lit, n, 0, 0); flush(); return o; }
            st[2]++;
            // one round of loads serves the usual sequence: 64 bytes before the match (backwards
            // extension), 64 after its first four (forwards extension: independent of how far
            // the backwards one goes, since the backtracked bytes match) and the pending literals
            const uint32_t cur0 = cur, cand0 = cand;
            const uint32_t mb0 = min(cur - lit, cand);
            const bool bok = l < mb0, fok = cur + 4 + l < match_lim, lok = lit + l < cur;
            const uint32_t bx = bok ? in[cur - 1 - l] : 0u, by = bok ? in[cand - 1 - l] : 1u;
            const uint32_t fx = fok ? in[cur + 4 + l] : 0u, fy = fok ? in[cand + 4 + l] : 1u;
            const uint32_t lb = lok ? in[lit + l] : 0u;
            {
                const uint64_t x = ballot(bx != by);
                uint32_t b = x ? ctz(x) : 64;
                cur -= b;
                cand -= b;
                while (b == 64) {   // extend backwards over the pending literals
                    const uint32_t mb = min(cur - lit, cand);
                    const bool eq = l < mb && in[cur - 1 - l] == in[cand - 1 - l];
                    const uint64_t y = ballot(!eq);
                    b = y ? ctz(y) : 64;
                    cur -= b;
                    cand -= b;
                }
            }
            const uint32_t m0 = cur, off = cur - cand;
            {
                const uint64_t x = ballot(fx != fy);
                uint32_t b = x ? ctz(x) : 64;
                cur = cur0 + 4 + b;
                cand = cand0 + 4 + b;
                while (b == 64) {   // extend forwards up to len - 6
                    const bool eq = cur + l < match_lim && in[cur + l] == in[cand + l];
                    const uint64_t y = ballot(!eq);
                    b = y ? ctz(y) : 64;
                    cur += b;
                    cand += b;
                }
            }
            const uint32_t h2 = hash(cur - 2);
            if (l == 0) vput(h2, cur - 2);
            tick(1);
            if (m0 - lit <= 64) emit_lits(lit, m0, lb, off, cur - m0);
            else emit(lit, m0, off, cur - m0);
            lit = cur;
            tick(2);
        }
    }
};

// ---- op runs: write_op (encode_oplog.rs:20-92); the ListOpMetrics merge (op_metrics.rs:235-293)
// is in encode_records_kernel
// the varint head of a written op run and its optional diff; op_end is the next cursor
DEV void op_code(uint4 r, uint32_t cursor, uint64_t &n, int64_t &diff, bool &has_diff, uint32_t &op_end) {
    const uint32_t start = r.x, end = r.y, len = end - start;
    const bool del = r.z & 1u, fwd = (r.z & 2u) || len == 1;
    const uint32_t op_start = (del && !fwd) ? end : start;
    op_end = (!del && fwd) ? end : start;
    diff = int64_t(op_start) - int64_t(cursor);
    uint64_t v;
    if (len != 1) v = del ? (uint64_t(len) * 2 + (fwd ? 1 : 0)) : len;
    else v = diff != 0 ? zz_old(diff) : 0;
    v = v * 2 + (del ? 1 : 0);
    v = v * 2 + (diff != 0 ? 1 : 0);
    v = v * 2 + (len != 1 ? 1 : 0);
    n = v;
    has_diff = len != 1 && diff != 0;
}

}  // namespace enc
}  // namespace dtgpu
