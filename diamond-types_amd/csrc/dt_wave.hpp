// Wave-level primitives shared by every kernel file: one definition, one name and one stated
// contract each.  A wave is 64 lanes (gfx950).  Everything is device-only and always inlined, so a
// kernel that uses a helper from here holds exactly the instructions a private copy would give.
// tests/device/wave_selftest.hip checks each primitive against its sequential definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define DEV __device__ __forceinline__

namespace dtgpu {
namespace wave {

typedef unsigned long long u64;   // what __ballot and the 64-bit bit intrinsics use

// ---- lanes and lane masks -----------------------------------------------------------------------
DEV uint32_t lane() { return __lane_id(); }
// v of lane l; l must be wave-uniform (v_readlane takes it from a scalar register).
DEV uint32_t rdl(uint32_t v, uint32_t l) { return uint32_t(__builtin_amdgcn_readlane(int(v), int(l))); }
DEV u64 rdl64(u64 v, uint32_t l) {
    return (u64(rdl(uint32_t(v >> 32), l)) << 32) | u64(rdl(uint32_t(v), l));
}
// v of the first active lane, in a scalar register.  Pinning a wave-uniform value this way makes
// the control flow that depends on it scalar (no exec-mask loops).
DEV uint32_t U(uint32_t v) { return uint32_t(__builtin_amdgcn_readfirstlane(int(v))); }
DEV u64 U64(u64 v) {   // (readfirstlane returns int: keep both halves unsigned)
    return (u64(U(uint32_t(v >> 32))) << 32) | u64(U(uint32_t(v)));
}
// v of lane src, src per lane (ds_bpermute).  Needs lane src active: an inactive source lane
// supplies 0, not its v, so call it with all 64 lanes active unless src is known to be active.
DEV uint32_t shfl(uint32_t v, uint32_t src) {
    return uint32_t(__builtin_amdgcn_ds_bpermute(int(src << 2), int(v)));
}
// Mask of the active lanes where p holds.  (The replay and the planner keep their flags as 0/1
// integers and hand them to __ballot as they are: through this bool parameter hipcc gives their
// kernels a different instruction stream, profiles/wave_header/text_identity.txt.)
DEV u64 ballot(bool p) { return __ballot(p); }
DEV uint32_t popc(u64 m) { return uint32_t(__popcll(m)); }
// Lowest / highest set bit of m; m must not be 0.
DEV uint32_t ctz(u64 m) { return uint32_t(__ffsll(m) - 1); }
DEV uint32_t last_lane(u64 m) { return 63u - uint32_t(__clzll((long long)m)); }
// Lanes below this one / below lane l (l >= 64: all lanes).
DEV u64 lt_mask() { return (1ull << lane()) - 1ull; }
DEV u64 lanes_below(uint32_t l) { return l >= 64 ? ~0ull : ((1ull << l) - 1ull); }
// Set bits of m below this lane (v_mbcnt: two VALU ops, no 64-bit shifts); = popc(m & lt_mask()).
DEV uint32_t bits_below(u64 m) {
    return __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
}

// ---- scans --------------------------------------------------------------------------------------
// Inclusive prefix scans along the wave in six DPP steps: row_shr 1, 2, 4, 8 scan each row of 16
// lanes, row_bcast 15 adds row 0's total to row 1 and row 2's to row 3, row_bcast 31 adds rows
// 0-1's total to rows 2 and 3.  A lane without a source reads 0, the identity of each operator.
// PRECONDITION, for every scan below: all 64 lanes active.  A DPP step reads its source lane's
// register whether or not that lane is active, and an inactive lane has not taken its own earlier
// steps, so under a partial mask the active lanes combine stale partial values.
// (The bodies are written out, not generated from one template: hipcc schedules a kernel around
// a nested helper differently, and this header must not change any kernel's instructions.)
// Prefix sum (mod 2^32).
DEV uint32_t scan_incl(uint32_t v) {
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x111, 0xF, 0xF, false));   // row_shr:1
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x112, 0xF, 0xF, false));   // row_shr:2
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x114, 0xF, 0xF, false));   // row_shr:4
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x118, 0xF, 0xF, false));   // row_shr:8
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x142, 0xA, 0xF, false));   // row_bcast:15
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x143, 0xC, 0xF, false));   // row_bcast:31
    return v;
}
// The same for lanes 0..31 only, one step fewer (lanes 32..63 are left with partial sums).
DEV uint32_t scan_incl32(uint32_t v) {
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x111, 0xF, 0xF, false));
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x112, 0xF, 0xF, false));
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x114, 0xF, 0xF, false));
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x118, 0xF, 0xF, false));
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x142, 0xA, 0xF, false));
    return v;
}
// Prefix maximum (unsigned).
DEV uint32_t scan_max(uint32_t v) {
    auto step = [&](uint32_t p) { v = v > p ? v : p; };
    step(uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x111, 0xF, 0xF, false)));
    step(uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x112, 0xF, 0xF, false)));
    step(uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x114, 0xF, 0xF, false)));
    step(uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x118, 0xF, 0xF, false)));
    step(uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x142, 0xA, 0xF, false)));
    step(uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x143, 0xC, 0xF, false)));
    return v;
}
// Prefix composition of boolean functions f_l: {0,1} -> {0,1}, each packed as f(0) | !f(1) << 1
// so that the identity is 0: lane l gets f_l o ... o f_0.
DEV uint32_t fn_pack(bool f0, bool f1) { return uint32_t(f0) | (uint32_t(!f1) << 1); }
DEV uint32_t compose_scan(uint32_t v) {
    auto step = [&](uint32_t p) {   // v := v o p
        const uint32_t m0 = v & 1u, m1 = ((v >> 1) & 1u) ^ 1u;
        const uint32_t p0 = p & 1u, p1 = ((p >> 1) & 1u) ^ 1u;
        v = (p0 ? m1 : m0) | (((p1 ? m1 : m0) ^ 1u) << 1);
    };
    step(uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x111, 0xF, 0xF, false)));
    step(uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x112, 0xF, 0xF, false)));
    step(uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x114, 0xF, 0xF, false)));
    step(uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x118, 0xF, 0xF, false)));
    step(uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x142, 0xA, 0xF, false)));
    step(uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x143, 0xC, 0xF, false)));
    return v;
}
// Sum over the wave, wave-uniform.  wave_sum is a scan (all 64 lanes active); wave_sum64 is a
// butterfly of lane exchanges with the same requirement.
DEV uint32_t wave_sum(uint32_t v) { return rdl(scan_incl(v), 63); }
DEV u64 wave_sum64(u64 v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// ---- fences -------------------------------------------------------------------------------------
// All are sequentially consistent and differ in scope only.  A wave's own memory operations of one
// kind complete in order; what a fence adds is that the compiler keeps them on their side of it
// and that the hardware waits or writes back as far as the scope needs.
// Wavefront scope, and no lane of the wave runs ahead of the others: LDS and global words that
// one lane of this wave wrote are read back by another lane of the same wave.
DEV void fence_wave() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); }
// Wavefront scope alone: only keeps the compiler from reordering the wave's LDS stores and loads.
DEV void fence_wave_nobarrier() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }
// Workgroup scope: this wave's stores are visible to later loads of every wave on the same CU
// (waits for the stores; the CU's L1 is shared, so nothing is invalidated).
DEV void fence_workgroup() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }
// Agent scope: this wave's stores and atomics have reached L2 and the CU's L1 lines are dropped,
// so later loads see what any other CU, or a memory-side atomic, wrote before.
DEV void fence_agent() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent"); }

// ---- scalar helpers -----------------------------------------------------------------------------
// (dt_host.hpp has the host's utf8_len)
DEV uint32_t utf8_len(uint8_t c) { return c < 0x80 ? 1 : (c & 0xE0) == 0xC0 ? 2 : (c & 0xF0) == 0xE0 ? 3 : 4; }
DEV u64 splitmix(u64 z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// CRC-32C combine (zlib's crc32_combine scheme over the reflected polynomial)
constexpr uint32_t CRC_POLY = 0x82F63B78u;
DEV uint32_t multmodp(uint32_t a, uint32_t b) {
    if (!a) return 0;
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}
DEV uint32_t x2nmodp(const uint32_t *x2n, u64 n, uint32_t k) {
    uint32_t p = 1u << 31;
    while (n) {
        if (n & 1) p = multmodp(x2n[k & 31], p);
        n >>= 1;
        k++;
    }
    return p;
}

}  // namespace wave
}  // namespace dtgpu
