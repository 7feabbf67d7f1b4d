// dt_merge.hip -- LV translation for the merge requests (dtgpu_merge.cpp).  A request's projection
// numbers Hist(from u merging) densely; its LV map is monotone and lives in the mark words the
// projection left (dt_mark.hpp: reach / nb per base entry).  merge_from_kernel takes each
// request's `from` into projected LVs before the planner runs; merge_records_kernel expands the
// reported commands of the finished replay into {base LV, transformed position} records.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dt_merge.hpp"
#include "dt_wave.hpp"

namespace dtgpu {
namespace mdev {
using namespace wave;

// The last index i < n with a[i * stride] <= key (a ascending, a[0] <= key, n >= 1).
DEV uint32_t find_le(const uint32_t *a, uint32_t stride, uint32_t n, uint32_t key) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a[size_t(mid) * stride] <= key) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(64) void merge_from_kernel(MergeParams P) {
    const uint32_t i = blockIdx.x;
    if (i >= P.n || !P.ok[i]) return;
    const HistDesc D = P.hd[i];
    const uint32_t ne = D.b_n_ent;
    if (!ne) return;
    const uint32_t *ent = P.b_ent + 2 * D.b_ent;
    const uint32_t *nb = P.scr + D.scr_off + ne;
    for (uint64_t k = P.from_off[i] + threadIdx.x; k < P.from_off[i + 1]; k += 64) {
        const uint32_t lv = P.from[k];
        const uint32_t e = find_le(ent, 2, ne, lv);
        P.from_out[k] = nb[e] + (lv - ent[2 * e]);
    }
}

// projected LV -> base LV: the last base entry whose new base LV is <= pl holds it (entries
// outside the history share the new base LV of the next included one, which comes after them).
DEV uint32_t to_base(const uint32_t *ent, const uint32_t *nb, uint32_t ne, uint32_t pl) {
    const uint32_t e = find_le(nb, 1, ne, pl);
    return ent[2 * e] + (pl - nb[e]);
}

constexpr uint32_t LONG_CMD = 16;   // longer commands are expanded by the whole wave

__global__ __launch_bounds__(64) void merge_records_kernel(MergeParams P) {
    const uint32_t i = blockIdx.x;
    if (i >= P.n) return;
    const uint32_t n_rec = P.n_rec[i];
    if (!n_rec) return;
    const HistDesc D = P.hd[i];
    const uint32_t ne = D.b_n_ent;
    if (!ne) return;
    const uint32_t l = lane();
    const uint32_t *ent = P.b_ent + 2 * D.b_ent;
    const uint32_t *nb = P.scr + D.scr_off + ne;
    const Cmd *cmds = P.cmds + P.cmd_off[i];
    const uint32_t *xf = P.xf + P.lv_off[i];
    uint32_t *rec = P.rec + 2 * P.rec_off[i];
    const uint32_t c1 = P.ncmd[i];
    uint32_t done = 0;   // records so far
    for (uint32_t c0 = P.first[i]; c0 < c1; c0 += 64) {
        const uint32_t c = c0 + l;
        Cmd q{CMD_TOG, 0, 0, 0};
        if (c < c1) q = cmds[c];
        const uint32_t len = (q.op & 15u) == CMD_TOG ? 0u : q.len;
        const uint32_t incl = scan_incl(len), off = done + incl - len;
        if (len && len <= LONG_CMD) {
            for (uint32_t j = 0; j < len; j++) {
                const uint32_t k = off + j;
                if (k < n_rec) { rec[2 * k] = to_base(ent, nb, ne, q.lv + j); rec[2 * k + 1] = xf[q.lv + j]; }
            }
        }
        for (u64 m = ballot(len > LONG_CMD); m; m &= m - 1) {
            const uint32_t s = ctz(m);
            const uint32_t lv0 = rdl(q.lv, s), n = rdl(len, s), o = rdl(off, s);
            for (uint32_t j = l; j < n; j += 64) {
                const uint32_t k = o + j;
                if (k < n_rec) { rec[2 * k] = to_base(ent, nb, ne, lv0 + j); rec[2 * k + 1] = xf[lv0 + j]; }
            }
        }
        done += rdl(incl, 63);
    }
}

}  // namespace mdev

int launch_merge_from(const MergeParams &p, void *stream) {
    if (!p.n) return OK;
    hipLaunchKernelGGL(mdev::merge_from_kernel, dim3(p.n), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), p);
    return launch_error() == hipSuccess ? OK : ErrHip;
}
int launch_merge_records(const MergeParams &p, void *stream) {
    if (!p.n) return OK;
    hipLaunchKernelGGL(mdev::merge_records_kernel, dim3(p.n), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), p);
    return launch_error() == hipSuccess ? OK : ErrHip;
}

}  // namespace dtgpu
