// Device self-test of diamond-types_amd/csrc/dt_wave.hpp: one workgroup of one full wave runs every
// primitive on a few hundred rounds of inputs, and the host compares each lane's result with the
// primitive's sequential definition.  Every call is made with all 64 lanes active (the loop bound
// and every branch are wave-uniform), which is the header's contract.
// Prints one line per mismatch (at most 20 per primitive) and a summary; exit status 0 = no
// mismatch, 1 = mismatches, 2 = no device or a HIP error.
// Build: make -C diamond-types_amd lib/wave_selftest
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dt_wave.hpp"

using namespace dtgpu::wave;

#define HIP_OK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) { \
    fprintf(stderr, "wave_selftest: %s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

// per round and lane
struct Out {
    uint32_t scan, scan32, max, comp, sum, rdl_, shfl_, rank, below, first, last, u;
    u64 sum64, rdl64_, ballot_, lb, u64_;
};

__global__ __launch_bounds__(64) void selftest(const uint32_t *x, const uint32_t *y, Out *out, uint32_t rounds) {
    const uint32_t l = lane();
    for (uint32_t r = 0; r < rounds; r++) {
        const uint32_t a = x[r * 64 + l], b = y[r * 64 + l];
        const u64 w = (u64(a) << 32) | b;
        Out o;
        o.scan = scan_incl(a);
        o.scan32 = scan_incl32(a);
        o.max = scan_max(a);
        o.comp = compose_scan(a & 3u);
        o.sum = wave_sum(a);
        o.sum64 = wave_sum64(w);
        o.rdl_ = rdl(a, r & 63u);
        o.rdl64_ = rdl64(w, (r * 7u) & 63u);
        o.shfl_ = shfl(a, b & 63u);
        const u64 m = ballot(a & 1u);
        o.ballot_ = m;
        o.rank = popc(m & lt_mask());
        o.below = bits_below(m);
        o.first = m ? ctz(m) : 64u;
        o.last = m ? last_lane(m) : 64u;
        o.lb = lanes_below(b % 67u);
        o.u = U(a);
        o.u64_ = U64(w);
        out[r * 64 + l] = o;
    }
}

// host-side xorshift64 for the random rounds
static u64 next_word(u64 s) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }

static int bad = 0;
template <typename T> static void expect(const char *what, uint32_t r, uint32_t l, T got, T want) {
    static const char *last = nullptr;
    static int shown = 0;
    if (got == want) return;
    bad++;
    if (last != what) { last = what; shown = 0; }
    if (shown++ < 20) printf("mismatch %s round %u lane %u: got 0x%llx want 0x%llx\n", what, r, l, (u64)got, (u64)want);
}

int main() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { fprintf(stderr, "wave_selftest: no HIP device\n"); return 2; }

    // rounds: all zeros, all ones, all 0xFFFFFFFF (the sum wraps), one non-zero lane at each row
    // seam with three values (1, 2 and 0xFFFFFFFF: compose_scan sees each non-identity function),
    // then seeded random words (every fourth round small values, so that sums do not wrap)
    const uint32_t seams[8] = {0, 15, 16, 31, 32, 47, 48, 63};
    const uint32_t seam_vals[3] = {1u, 2u, 0xFFFFFFFFu};
    const uint32_t R = 3 + 8 * 3 + 300;
    std::vector<uint32_t> x(R * 64, 0u), y(R * 64);
    uint32_t r = 1;
    for (uint32_t l = 0; l < 64; l++) { x[r * 64 + l] = 1u; x[(r + 1) * 64 + l] = 0xFFFFFFFFu; }
    r = 3;
    for (uint32_t s = 0; s < 8; s++)
        for (uint32_t v = 0; v < 3; v++) x[r++ * 64 + seams[s]] = seam_vals[v];
    u64 seed = 0xD1A0C0DEull;
    for (; r < R; r++)
        for (uint32_t l = 0; l < 64; l++) {
            seed = next_word(seed);
            x[r * 64 + l] = (r & 3u) == 3u ? uint32_t(seed >> 20) % 1000u : uint32_t(seed >> 20);
        }
    for (auto &v : y) { seed = next_word(seed); v = uint32_t(seed >> 20); }

    uint32_t *dx, *dy;
    Out *dout;
    std::vector<Out> o(R * 64);
    HIP_OK(hipMalloc(&dx, x.size() * 4));
    HIP_OK(hipMalloc(&dy, y.size() * 4));
    HIP_OK(hipMalloc(&dout, o.size() * sizeof(Out)));
    HIP_OK(hipMemcpy(dx, x.data(), x.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dy, y.data(), y.size() * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(selftest, dim3(1), dim3(64), 0, 0, dx, dy, dout, R);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(o.data(), dout, o.size() * sizeof(Out), hipMemcpyDeviceToHost));

    for (r = 0; r < R; r++) {
        const uint32_t *a = &x[r * 64], *b = &y[r * 64];
        const Out *g = &o[r * 64];
        uint32_t total = 0;
        u64 total64 = 0, m = 0;
        for (uint32_t l = 0; l < 64; l++) {
            total += a[l];
            total64 += (u64(a[l]) << 32) | b[l];
            m |= u64(a[l] & 1u) << l;
        }
        uint32_t first = 64, last = 64;
        for (uint32_t l = 0; l < 64; l++) if ((m >> l) & 1) { if (first == 64) first = l; last = l; }
        uint32_t sum = 0, mx = 0, rank = 0;
        int a0 = 0, a1 = 1;   // the composition so far, applied to 0 and to 1
        for (uint32_t l = 0; l < 64; l++) {
            sum += a[l];
            mx = a[l] > mx ? a[l] : mx;
            const uint32_t f = a[l] & 3u;
            const int f0 = f & 1, f1 = ((f >> 1) & 1) ^ 1;
            const int n0 = a0 ? f1 : f0, n1 = a1 ? f1 : f0;
            a0 = n0; a1 = n1;
            const uint32_t rl = r & 63u, rl64 = (r * 7u) & 63u, k = b[l] % 67u;
            expect("scan_incl", r, l, g[l].scan, sum);
            if (l < 32) expect("scan_incl32", r, l, g[l].scan32, sum);
            expect("scan_max", r, l, g[l].max, mx);
            expect("compose_scan", r, l, g[l].comp, uint32_t(a0) | (uint32_t(a1 ^ 1) << 1));
            expect("wave_sum", r, l, g[l].sum, total);
            expect("wave_sum64", r, l, g[l].sum64, total64);
            expect("rdl", r, l, g[l].rdl_, a[rl]);
            expect("rdl64", r, l, g[l].rdl64_, (u64(a[rl64]) << 32) | b[rl64]);
            expect("shfl", r, l, g[l].shfl_, a[b[l] & 63u]);
            expect("ballot", r, l, g[l].ballot_, m);
            expect("popc(ballot & lt_mask)", r, l, g[l].rank, rank);
            expect("bits_below", r, l, g[l].below, rank);
            expect("ctz", r, l, g[l].first, first);
            expect("last_lane", r, l, g[l].last, last);
            expect("lanes_below", r, l, g[l].lb, k >= 64 ? ~0ull : (1ull << k) - 1ull);
            expect("U", r, l, g[l].u, a[0]);
            expect("U64", r, l, g[l].u64_, (u64(a[0]) << 32) | b[0]);
            rank += a[l] & 1u;
        }
    }
    printf("wave_selftest: %u rounds of 64 lanes, %d mismatches\n", R, bad);
    return bad ? 1 : 0;
}
