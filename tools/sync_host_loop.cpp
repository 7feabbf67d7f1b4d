// sync_host_loop.cpp -- the baseline of tools/bench_sync.py: per request, the host's
// dtgpu_oplog_intersect_summary and then dtgpu_oplog_encode from the common frontier, over a batch
// of sync hellos on native threads (no interpreter in the timed window).  Host code only; the tool
// builds it into a shared library and passes it the two functions' addresses.
//
//   g++ -O2 -std=c++17 -shared -fPIC -pthread -Iinclude tools/sync_host_loop.cpp -o sync_host_loop.so
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <thread>
#include <vector>

#include "dtgpu.h"

typedef int (*intersect_fn)(const void *oplog, const dtgpu_summaries *s, size_t i, uint64_t *frontier, size_t fcap,
                            size_t *n_frontier, uint64_t *triples, size_t tcap, size_t *n_triples);
typedef int (*encode_fn)(const void *oplog, const uint64_t *from, size_t n_from, uint32_t flags, uint8_t *out,
                         size_t cap, size_t *out_len);

// Request i of s against oplogs[s->doc[i]]; the patch goes to arena[aoff[i] .. aoff[i + 1]).
// `threads` threads take contiguous slices, `reps` times over; returns the wall seconds of it all,
// thread start and join included.  len[i], status[i] and n_rem[i] are the last repetition's.
extern "C" double sync_host_loop(intersect_fn intersect, encode_fn encode, void *const *oplogs, const dtgpu_summaries *s,
                                 size_t n, uint32_t flags, int threads, int reps, uint8_t *arena, const size_t *aoff,
                                 size_t *len, int *status, size_t *n_rem) {
    if (threads < 1) threads = 1;
    const size_t step = (n + size_t(threads) - 1) / size_t(threads);
    const auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < reps; r++) {
        std::vector<std::thread> pool;
        for (size_t lo = 0; lo < n; lo += step) {
            const size_t hi = lo + step < n ? lo + step : n;
            pool.emplace_back([=] {
                uint64_t front[64];
                std::vector<uint64_t> rem(3 * 64);
                for (size_t i = lo; i < hi; i++) {
                    size_t nf = 0, nt = 0;
                    len[i] = 0;
                    const void *o = oplogs[s->doc[i]];
                    status[i] = intersect(o, s, i, front, 64, &nf, rem.data(), rem.size() / 3, &nt);
                    if (!status[i] && nt > rem.size() / 3) {   // more remainder records than the buffer: once more
                        rem.resize(3 * nt);
                        status[i] = intersect(o, s, i, front, 64, &nf, rem.data(), nt, &nt);
                    }
                    n_rem[i] = nt;
                    if (!status[i] && nf > 64) status[i] = DTGPU_DECODE_DEFER;
                    if (!status[i]) status[i] = encode(o, front, nf, flags, arena + aoff[i], aoff[i + 1] - aoff[i], &len[i]);
                }
            });
        }
        for (auto &t : pool) t.join();
    }
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
