#!/usr/bin/env python3
"""Patches since a version for a batch of resident documents: DecodeBatch.encode_from on the device
(B) against the loop of host dtgpu_oplog_encode calls on 16 native threads (A), alternating in one
process, every run listed.

A is the only way to get these bytes without the batched encoder, and its code is unchanged by it.
The loop runs in tools/patch_host_loop.cpp (std::thread over the C ABI, each patch written into
its slot of one preallocated arena): no interpreter inside the timed window.  Its host oplogs are
loaded outside the timing (load time listed).  B's documents are decoded on the device once,
outside the timing: the resident oplog is the premise.  Both sides are warmed up at the timed
size; a timed window repeats the whole batch `reps` times (a few tenths of a second) and the
figures are per batch.  B reports the synchronised call time and the two launches' device time
(HIP events).  Apart from the timed runs: the time to copy every patch to the host, a sample of
build waves' cycles per phase (DTGPU_PATCH_PROF), and the mark launch with the sweep's earlier
agent-scope fence (DTGPU_MARK_AGENT_FENCE).  The two sides' bytes are compared for every request.

    python tools/bench_patches.py [--out profiles/patches/bench_patches.json]
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diamond-types_amd"))
import dt_amd   # noqa: E402

THREADS = 16
PHASES = ("pieces_edges", "walk", "agent_txn_records", "op_runs", "text_gather", "lz4", "write_crc")


def host_loop_lib():
    """tools/patch_host_loop.cpp as a shared library beside libdtgpu.so (built when missing or stale)."""
    src = os.path.join(ROOT, "tools", "patch_host_loop.cpp")
    so = os.path.join(os.path.dirname(dt_amd.LIB_PATH), "patch_host_loop.so")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", src, "-o", so])
    H = ctypes.CDLL(so)
    H.patch_host_loop.restype = ctypes.c_double
    H.patch_host_loop.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int, ctypes.c_int] + \
                                 [ctypes.c_void_p] * 4
    return H


class HostLoop:
    """The requests flattened once for the native loop; run(reps) -> (seconds per batch, patches)."""

    def __init__(self, oplogs, docs, vs, flags, lens):
        n = len(vs)
        self.n, self.flags, self.H = n, flags, host_loop_lib()
        self.fn = ctypes.cast(dt_amd.lib().dtgpu_oplog_encode, ctypes.c_void_p)
        self.oplogs = (ctypes.c_void_p * len(oplogs))(*[o._h for o in oplogs])
        self.doc = (ctypes.c_uint32 * n)(*docs)
        flat, off = [], [0]
        for v in vs:
            flat.extend(v)
            off.append(len(flat))
        self.versions = (ctypes.c_uint64 * max(1, len(flat)))(*flat)
        self.voff = (ctypes.c_size_t * (n + 1))(*off)
        aoff = [0]
        for k in lens:   # each slot holds exactly the patch the device wrote (a longer one is an error status)
            aoff.append(aoff[-1] + k)
        self.aoff_py = aoff
        self.aoff = (ctypes.c_size_t * (n + 1))(*aoff)
        self.arena = ctypes.create_string_buffer(max(1, aoff[-1]))
        self.len = (ctypes.c_size_t * n)()
        self.status = (ctypes.c_int * n)()

    def run(self, reps):
        s = self.H.patch_host_loop(self.fn, self.oplogs, self.doc, self.versions, self.voff, self.n, self.flags, THREADS,
                                   reps, self.arena, self.aoff, self.len, self.status)
        bad = [i for i in range(self.n) if self.status[i] or self.len[i] != self.aoff_py[i + 1] - self.aoff_py[i]]
        if bad:
            raise RuntimeError(f"host encode {bad[0]}: status {self.status[bad[0]]}, {self.len[bad[0]]} bytes")
        return s / reps, self.arena.raw[:self.aoff_py[-1]]


def device_calls(d, docs, vs, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        pb = d.encode_from(docs, vs)   # returns with the stream synchronised
    t1 = time.perf_counter()
    prof = pb.profile(0)
    return (t1 - t0) / reps, prof[1] / 1000.0, prof[2] / 1000.0, pb


def with_env(name, fn):
    os.environ[name] = "1"
    try:
        return fn()
    finally:
        del os.environ[name]


def bench(label, name, n_docs, docs, make_versions, reps, rounds=3):
    with open(os.path.join(ROOT, "tests", "golden", "benchmark_data", name + ".dt"), "rb") as f:
        data = f.read()
    t = time.perf_counter()
    oplogs = [dt_amd.ListOpLog.load_from(data) for _ in range(n_docs)]
    load_s = time.perf_counter() - t
    vs = make_versions(oplogs[0])
    d = dt_amd.DecodeBatch([data] * n_docs)
    d.run()
    flags = dt_amd.ENCODE_PATCH.flags()
    # warm-up at the timed size; the device's patches size the host loop's arena
    _, _, _, pb = device_calls(d, docs, vs, 1)
    t = time.perf_counter()
    got = [pb.patch(i) for i in range(len(vs))]
    fetch_s = time.perf_counter() - t
    host = HostLoop(oplogs, docs, vs, flags, [len(p) for p in got])
    _, want = host.run(1)
    if want != b"".join(got):
        raise AssertionError(f"{label}: the device's patches differ from the host encoder's")
    rows = []
    for _ in range(rounds):
        ta, _ = host.run(reps)
        tb, mark_ms, build_ms, _ = device_calls(d, docs, vs, reps)
        rows.append({"host_loop_16_threads_s": ta, "device_call_s": tb, "mark_kernel_ms": mark_ms, "build_kernel_ms": build_ms})
    # apart from the timed runs: phase cycles of a sample of build waves, and the sweep's earlier fence
    pb = with_env("DTGPU_PATCH_PROF", lambda: d.encode_from(docs, vs))
    prof = [pb.profile(i) for i in range(0, len(vs), max(1, len(vs) // 16))]
    cycles = {k: sum(p[4 + j] for p in prof) / len(prof) for j, k in enumerate(PHASES)}
    agent_fence = [with_env("DTGPU_MARK_AGENT_FENCE", lambda: device_calls(d, docs, vs, 1))[1] for _ in range(3)]
    col = lambda k: [r[k] for r in rows]
    ha, de = col("host_loop_16_threads_s"), col("device_call_s")
    res = {"workload": label, "document": name, "resident_documents": n_docs, "requests": len(vs),
           "batches_per_timed_window": reps, "patch_bytes_first": len(got[0]), "patch_bytes_total": len(want),
           "host_oplog_load_s": load_s, "device_fetch_all_patches_s": fetch_s, "runs": rows,
           "best_host_loop_16_threads_s": min(ha), "median_host_loop_16_threads_s": statistics.median(ha),
           "best_device_call_s": min(de), "median_device_call_s": statistics.median(de),
           "ratio_host_over_device_call_median": statistics.median(ha) / statistics.median(de),
           "device_ahead_in_every_run": all(b < a for a, b in zip(ha, de)),
           "device_behind_in_every_run": all(b > a for a, b in zip(ha, de)),
           "build_wave_cycles": cycles,
           "mark_kernel_ms_with_agent_scope_fence": agent_fence}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patches", "bench_patches.json"))
    ap.add_argument("--requests", type=int, default=10000)
    args = ap.parse_args()
    if dt_amd.device_count() < 1:
        raise SystemExit("bench_patches: no HIP device visible (the engine has no CPU fallback)")
    k = args.requests
    n_docs = min(100, k)
    spread = [i % n_docs for i in range(k)]
    rng = random.Random(59)
    results = [
        bench("friendsforever, from = [0.99 n]", "friendsforever", n_docs, spread, lambda o: [[int(len(o) * 0.99)]] * k, 16),
        bench("friendsforever, from = [0.5 n]", "friendsforever", n_docs, spread, lambda o: [[int(len(o) * 0.5)]] * k, 4),
        bench("git-makefile, 64 versions", "git-makefile", 1, [0] * 64,
              lambda o: [o.dominators(rng.sample(range(len(o)), rng.choice([1, 2, 3]))) for _ in range(64)], 8),
    ]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/bench_patches.py", "host_threads": THREADS, "workloads": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
