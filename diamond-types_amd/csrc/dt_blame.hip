// dt_blame.hip -- batched blame on MI355X (gfx950): each document's text as maximal runs
// (lv, len, agent, seq), from the lists the checkout pass leaves behind.  See dt_blame.hpp.
//
// Kernels, all integer and memory work:
//   blame_len_kernel    thread per document: the entries of its final source list, before the
//                       combine step rewrites a group of one's result
//   blame_bits_kernel   workgroup per document: one bit per LV, set where an agent run starts
//                       whose (agent, seq) does not continue the run before it
//   blame_runs_kernel   workgroup per document, counting or emitting: head flags over the final
//                       list (tracker) or over the final pieces and the boundary bits inside them
//                       (fast-forward), a block scan for the run slots, one 16-byte run per head
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "dt_blame.hpp"
#include "dt_host.hpp"
#include "dt_wave.hpp"

namespace dtgpu {
namespace blame {
using namespace wave;

constexpr uint32_t BT = 256;   // threads per document

// Exclusive prefix sum over the workgroup (every thread calls it); total = the sum.  s_w holds
// BT / 64 words.  Ends with a barrier.
DEV uint32_t block_scan(uint32_t x, uint32_t *s_w, uint32_t &total) {
    const uint32_t w = threadIdx.x / 64;
    const uint32_t inc = scan_incl(x);
    if (lane() == 63) s_w[w] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (uint32_t k = 0; k < BT / 64; k++) {
        const uint32_t v = s_w[k];
        base += k < w ? v : 0;
        tot += v;
    }
    total = tot;
    __syncthreads();
    return base + inc - x;
}

__global__ __launch_bounds__(256) void blame_len_kernel(BlameParams P) {
    const uint32_t d = blockIdx.x * 256 + threadIdx.x;
    if (d >= P.n_docs) return;
    const BlameDoc D = P.docs[d];
    if (D.kind != BLAME_TRACKER) return;
    const DocResult &r = P.results[D.last];
    P.len[d] = r.status ? 0u : min(r.out_len, D.cap);
}

// Agent run k of a document: quads (lv_start, name rank, seq_start, agent), ascending lv_start.
DEV uint4 arun(const uint32_t *ar, uint32_t k) { return reinterpret_cast<const uint4 *>(ar)[k]; }
// The agent run holding lv (n >= 1, the first run starts at LV 0).
DEV uint32_t arun_of(const uint32_t *ar, uint32_t n, uint32_t lv) {
    uint32_t lo = 0, hi = n;   // answer in [lo, hi)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (ar[4 * mid] <= lv) lo = mid; else hi = mid;
    }
    return lo;
}
DEV BlameRun run_at(const uint32_t *ar, uint32_t n, uint32_t lv, uint32_t start) {
    const uint4 a = arun(ar, arun_of(ar, n, lv));
    return BlameRun{lv, start, a.w, a.z + (lv - a.x)};   // len holds the run's first character for now
}

__global__ __launch_bounds__(BT) void blame_bits_kernel(BlameParams P) {
    const BlameDoc D = P.docs[blockIdx.x];
    if (D.kind == BLAME_NONE) return;
    const uint32_t t = threadIdx.x;
    uint32_t *bits = P.bits + D.bits_off;
    const uint32_t nw = (D.n_lv + 31) / 32;
    for (uint32_t i = t; i < nw; i += BT) bits[i] = 0;
    __syncthreads();
    const uint32_t *ar = P.aruns + D.arun_off;
    for (uint32_t k = 1 + t; k < D.n_aruns; k += BT) {
        const uint4 a = arun(ar, k - 1), b = arun(ar, k);
        if (b.x < D.n_lv && (b.w != a.w || b.z != a.z + (b.x - a.x))) atomicOr(bits + (b.x >> 5), 1u << (b.x & 31));
    }
}

DEV bool bit_at(const uint32_t *bits, uint32_t lv) { return (bits[lv >> 5] >> (lv & 31)) & 1u; }
// Set bits of the LVs [lo, hi).
DEV uint32_t bits_in(const uint32_t *bits, uint32_t lo, uint32_t hi) {
    uint32_t n = 0;
    for (uint32_t w = lo >> 5; lo < hi; w++) {
        const uint32_t end = min(hi, (w + 1) << 5);
        uint32_t m = bits[w] >> (lo & 31);
        if (end - lo < 32) m &= (1u << (end - lo)) - 1u;
        n += __popc(m);
        lo = end;
    }
    return n;
}

// The runs' first characters (held in len) to lengths: run k ends where run k + 1 starts, the last
// one at the text's end.  Every thread of the workgroup calls it.
DEV void starts_to_lens(BlameRun *runs, uint32_t n, uint32_t n_chars) {
    __syncthreads();   // the emit loop's stores
    for (uint32_t k0 = 0; k0 < n; k0 += BT) {
        const uint32_t k = k0 + threadIdx.x;
        uint32_t a = 0, b = 0;
        if (k < n) { a = runs[k].len; b = k + 1 < n ? runs[k + 1].len : n_chars; }
        __syncthreads();
        if (k < n) runs[k].len = b - a;
    }
}

template <bool EMIT>
__global__ __launch_bounds__(BT) void blame_runs_kernel(BlameParams P) {
    __shared__ uint32_t s_w[BT / 64], s_n;
    const uint32_t d = blockIdx.x, t = threadIdx.x;
    const BlameDoc D = P.docs[d];
    const bool ok = D.kind != BLAME_NONE && P.results[d].status == 0 && D.n_aruns != 0;
    const uint32_t *ar = P.aruns + D.arun_off;
    const uint32_t *bits = P.bits + D.bits_off;
    BlameRun *runs = EMIT ? P.runs + P.run_off[d] : nullptr;
    const uint32_t lim = EMIT ? P.count[d] : 0u;   // the slots the counting pass reserved
    uint32_t carry = 0, n_chars = 0;
    if (ok && D.kind == BLAME_TRACKER) {
        const uint32_t *L = P.src + D.src_off;
        if (t == 0) {   // the list ends at the first entry that is still a placeholder (monotone)
            uint32_t lo = 0, hi = P.len[d];
            while (lo < hi) {
                const uint32_t mid = (lo + hi) / 2;
                if (L[mid] & SEG_PHANTOM) hi = mid; else lo = mid + 1;
            }
            s_n = lo;
        }
        __syncthreads();
        n_chars = s_n;
        for (uint32_t r0 = 0; r0 < n_chars; r0 += BT) {
            const uint32_t i = r0 + t;
            uint32_t head = 0, e = 0;
            if (i < n_chars) {
                e = L[i];
                head = i == 0 || e != L[i - 1] + 1 || (e < D.n_lv && bit_at(bits, e)) ? 1u : 0u;
            }
            uint32_t tot = 0;
            const uint32_t ex = block_scan(head, s_w, tot);
            if (EMIT && head && e < D.n_lv && carry + ex < lim) runs[carry + ex] = run_at(ar, D.n_aruns, e, i);
            carry += tot;
        }
    } else if (ok && D.kind == BLAME_FF) {
        const FFDoc &F = P.ff_docs[D.last];
        const bool odd = (F.levels & 1u) != 0;
        const uint4 *pc = reinterpret_cast<const uint4 *>(odd ? P.pb : P.pa) + F.piece_off;
        const uint32_t nf = (odd ? P.cb : P.ca)[F.first_seg];
        if (nf) { const uint4 z = pc[nf - 1]; n_chars = z.z + z.y; }
        for (uint32_t r0 = 0; r0 < nf; r0 += BT) {
            const uint32_t i = r0 + t;
            uint4 p = make_uint4(0, 0, 0, 0);
            uint32_t head = 0, cnt = 0;
            if (i < nf) {
                p = pc[i];
                if (p.x < D.n_lv && p.y && p.y <= D.n_lv - p.x) {   // (a placeholder piece fails the document)
                    head = 1;
                    if (i) { const uint4 q = pc[i - 1]; head = q.x + q.y != p.x || bit_at(bits, p.x) ? 1u : 0u; }
                    cnt = head + bits_in(bits, p.x + 1, p.x + p.y);
                }
            }
            uint32_t tot = 0;
            const uint32_t ex = block_scan(cnt, s_w, tot);
            if (EMIT && cnt) {   // the piece's own head, then a run at every boundary inside it
                uint32_t o = carry + ex;
                if (head && o < lim) runs[o++] = run_at(ar, D.n_aruns, p.x, p.z);
                for (uint32_t lv = p.x + 1; lv < p.x + p.y;) {
                    const uint32_t m = bits[lv >> 5] >> (lv & 31);
                    if (!m) { lv = (lv | 31u) + 1; continue; }
                    lv += __ffs(m) - 1;
                    if (lv >= p.x + p.y || o >= lim) break;
                    runs[o++] = run_at(ar, D.n_aruns, lv, p.z + (lv - p.x));
                    lv++;
                }
            }
            carry += tot;
        }
    }
    if (EMIT) {
        starts_to_lens(runs, min(carry, lim), n_chars);
    } else if (t == 0) {
        P.count[d] = carry;
        P.count[P.n_docs + d] = carry ? n_chars : 0u;
    }
}

}  // namespace blame

int launch_blame_len(const BlameParams &p, void *stream) {
    if (!p.n_docs) return OK;
    hipLaunchKernelGGL(blame::blame_len_kernel, dim3((p.n_docs + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p);
    return launch_error() == hipSuccess ? OK : ErrHip;
}
int launch_blame_count(const BlameParams &p, void *stream) {
    if (!p.n_docs) return OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(blame::blame_bits_kernel, dim3(p.n_docs), dim3(blame::BT), 0, s, p);
    hipLaunchKernelGGL(blame::blame_runs_kernel<false>, dim3(p.n_docs), dim3(blame::BT), 0, s, p);
    return launch_error() == hipSuccess ? OK : ErrHip;
}
int launch_blame_emit(const BlameParams &p, void *stream) {
    if (!p.n_docs) return OK;
    hipLaunchKernelGGL(blame::blame_runs_kernel<true>, dim3(p.n_docs), dim3(blame::BT), 0, reinterpret_cast<hipStream_t>(stream), p);
    return launch_error() == hipSuccess ? OK : ErrHip;
}

}  // namespace dtgpu
