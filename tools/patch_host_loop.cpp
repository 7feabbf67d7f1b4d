// patch_host_loop.cpp -- the baseline of tools/bench_patches.py: the loop of host dtgpu_oplog_encode
// calls over a batch of requests on native threads (no interpreter in the timed window).  Host
// code only; the tool builds it into a shared library and passes it the encoder's address.
//
//   g++ -O2 -std=c++17 -shared -fPIC -pthread tools/patch_host_loop.cpp -o patch_host_loop.so
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <thread>
#include <vector>

typedef int (*encode_fn)(const void *oplog, const uint64_t *from, size_t n_from, uint32_t flags, uint8_t *out,
                         size_t cap, size_t *out_len);

// Request i: oplogs[doc[i]] from versions[voff[i] .. voff[i + 1]) into arena[aoff[i] .. aoff[i + 1]).
// `threads` threads take contiguous slices, `reps` times over; returns the wall seconds of it all,
// thread start and join included.  len[i] and status[i] are the last repetition's.
extern "C" double patch_host_loop(encode_fn encode, void *const *oplogs, const uint32_t *doc, const uint64_t *versions,
                                  const size_t *voff, size_t n, uint32_t flags, int threads, int reps, uint8_t *arena,
                                  const size_t *aoff, size_t *len, int *status) {
    if (threads < 1) threads = 1;
    const size_t step = (n + size_t(threads) - 1) / size_t(threads);
    const auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < reps; r++) {
        std::vector<std::thread> pool;
        for (size_t lo = 0; lo < n; lo += step) {
            const size_t hi = lo + step < n ? lo + step : n;
            pool.emplace_back([=] {
                for (size_t i = lo; i < hi; i++) {
                    len[i] = 0;
                    status[i] = encode(oplogs[doc[i]], versions + voff[i], voff[i + 1] - voff[i], flags, arena + aoff[i],
                                       aoff[i + 1] - aoff[i], &len[i]);
                }
            });
        }
        for (auto &t : pool) t.join();
    }
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
