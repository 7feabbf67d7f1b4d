#!/usr/bin/env python3
"""A batch of sync hellos answered for resident documents: every request is a peer's version summary
(the summary of the document's history at some version), the answer is the common frontier, the
remainder and the `.dt` patch of what the peer lacks.  Three legs on the same requests, alternating
in one process, every run listed:

  fused     DecodeBatch.sync: dtgpu_decode_encode_from_summaries, the LV sets stay in HBM
  two_call  DecodeBatch.intersect, the frontiers read back to the host, then DecodeBatch.encode_from
  host      per request dtgpu_oplog_intersect_summary + dtgpu_oplog_encode on 16 native threads
            (tools/sync_host_loop.cpp: no interpreter inside the timed window)

The host leg's oplogs are loaded outside the timing (100 distinct ones stand behind the documents'
indexes, which only spares memory and helps the host's caches); the device legs' documents are decoded on the
device once, outside the timing: the resident oplog is the premise.  Each leg is warmed up at the
timed size; the flattened summaries are packed once and reused by all three.  The device legs report
the synchronised call time and the kernels' device time (HIP events).  The bytes and the frontiers
of the three legs are compared for every request.  A measurement tool: no threshold is attached.

    python tools/bench_sync.py [--out profiles/sync/bench_sync.json] [--requests 10000]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diamond-types_amd"))
import dt_amd   # noqa: E402

THREADS = 16
HOST_OPLOGS = 100   # distinct host oplogs behind the resident documents' indexes (memory; favours the host's caches)


def host_loop_lib():
    """tools/sync_host_loop.cpp as a shared library beside libdtgpu.so (built when missing or stale)."""
    src = os.path.join(ROOT, "tools", "sync_host_loop.cpp")
    so = os.path.join(os.path.dirname(dt_amd.LIB_PATH), "sync_host_loop.so")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-I" + os.path.join(ROOT, "include"),
                               src, "-o", so])
    H = ctypes.CDLL(so)
    H.sync_host_loop.restype = ctypes.c_double
    H.sync_host_loop.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int, ctypes.c_int] + \
                                [ctypes.c_void_p] * 5
    return H


class HostLoop:
    def __init__(self, oplogs, S, n, flags, lens):
        self.n, self.flags, self.S, self.H = n, flags, S, host_loop_lib()
        L = dt_amd.lib()
        self.fi = ctypes.cast(L.dtgpu_oplog_intersect_summary, ctypes.c_void_p)
        self.fe = ctypes.cast(L.dtgpu_oplog_encode, ctypes.c_void_p)
        self.oplogs = (ctypes.c_void_p * len(oplogs))(*[o._h for o in oplogs])
        aoff = [0]
        for k in lens:   # each slot holds exactly the patch the device wrote (a longer one is an error status)
            aoff.append(aoff[-1] + k)
        self.aoff_py = aoff
        self.aoff = (ctypes.c_size_t * (n + 1))(*aoff)
        self.arena = ctypes.create_string_buffer(max(1, aoff[-1]))
        self.len, self.status, self.n_rem = (ctypes.c_size_t * n)(), (ctypes.c_int * n)(), (ctypes.c_size_t * n)()

    def run(self, reps):
        s = self.H.sync_host_loop(self.fi, self.fe, self.oplogs, ctypes.addressof(self.S), self.n, self.flags, THREADS, reps,
                                  self.arena, self.aoff, self.len, self.status, self.n_rem)
        bad = [i for i in range(self.n) if self.status[i] or self.len[i] != self.aoff_py[i + 1] - self.aoff_py[i]]
        if bad:
            raise RuntimeError(f"host sync {bad[0]}: status {self.status[bad[0]]}, {self.len[bad[0]]} bytes")
        return s / reps, self.arena.raw[:self.aoff_py[-1]]


def fused(d, S, n, flags):
    ms, hp, hx = ctypes.c_float(), ctypes.c_void_p(), ctypes.c_void_p()
    t0 = time.perf_counter()
    st = dt_amd.lib().dtgpu_decode_encode_from_summaries(d._h, ctypes.byref(S), n, flags, ctypes.byref(ms), ctypes.byref(hp),
                                                         ctypes.byref(hx))
    t = time.perf_counter() - t0
    if st:
        raise RuntimeError(f"fused call: status {st}")
    return t, ms.value, dt_amd.PatchBatch(hp, n, ms.value), dt_amd.IntersectBatch(hx, n, ms.value, None)


def two_call(d, S, n, flags):
    """intersect; every frontier to the host (one C call per request, as a caller has to); encode_from."""
    L = dt_amd.lib()
    ms0, ms1, hx, hp = ctypes.c_float(), ctypes.c_float(), ctypes.c_void_p(), ctypes.c_void_p()
    flat, off = (ctypes.c_uint64 * (64 * n))(), (ctypes.c_size_t * (n + 1))()
    k = ctypes.c_size_t()
    t0 = time.perf_counter()
    st = L.dtgpu_decode_intersect(d._h, ctypes.byref(S), n, ctypes.byref(ms0), ctypes.byref(hx))
    if st:
        raise RuntimeError(f"intersect: status {st}")
    x = dt_amd.IntersectBatch(hx, n, ms0.value, None)
    t1 = time.perf_counter()
    at = 0
    for i in range(n):
        L.dtgpu_intersect_result(hx, i, ctypes.cast(ctypes.byref(flat, 8 * at), ctypes.POINTER(ctypes.c_uint64)), 64, ctypes.byref(k))
        at += k.value
        off[i + 1] = at
    t2 = time.perf_counter()
    st = L.dtgpu_decode_encode_from(d._h, S.doc, flat, off, n, flags, ctypes.byref(ms1), ctypes.byref(hp))
    t3 = time.perf_counter()
    if st:
        raise RuntimeError(f"encode_from: status {st}")
    return {"call_s": t3 - t0, "intersect_call_s": t1 - t0, "frontiers_to_host_s": t2 - t1, "encode_from_call_s": t3 - t2,
            "intersect_kernels_ms": ms0.value, "patch_kernels_ms": ms1.value}, dt_amd.PatchBatch(hp, n, ms1.value), x


def bench(label, name, n_docs, docs, version_of, rounds=3, host_reps=1):
    with open(os.path.join(ROOT, "tests", "golden", "benchmark_data", name + ".dt"), "rb") as f:
        data = f.read()
    t = time.perf_counter()
    distinct = [dt_amd.ListOpLog.load_from(data) for _ in range(min(n_docs, HOST_OPLOGS))]
    load_s = time.perf_counter() - t
    oplogs = [distinct[i % len(distinct)] for i in range(n_docs)]   # the host leg only reads them
    o = oplogs[0]
    n = len(docs)
    v = version_of(o)
    hello = dt_amd.normalize_summary(o.history([v]).summarize_versions())
    want_front = o.dominators([v])
    S, _ = dt_amd._pack_summaries([hello] * n, docs)
    d = dt_amd.DecodeBatch([data] * n_docs)
    d.run()
    flags = dt_amd.ENCODE_PATCH.flags()
    # warm-up at the timed size; the device's patches size the host loop's arena; all legs must agree
    _, _, pb, x = fused(d, S, n, flags)
    got = [pb.patch(i) for i in range(n)]
    if any(x.frontier(i) != want_front or x.remainder_records(i) for i in range(0, n, max(1, n // 64))):
        raise AssertionError(f"{label}: the fused call's intersection is not the hello's version")
    _, pb2, x2 = two_call(d, S, n, flags)
    if any(pb2.patch(i) != got[i] for i in range(0, n, max(1, n // 64))):
        raise AssertionError(f"{label}: the two-call path's patches differ from the fused call's")
    host = HostLoop(oplogs, S, n, flags, [len(p) for p in got])
    _, want = host.run(1)
    if want != b"".join(got):
        raise AssertionError(f"{label}: the device's patches differ from the host path's")
    prof = x.profile(0)
    rows = []
    for _ in range(rounds):
        th, _ = host.run(host_reps)
        tf, fms, pbf, xf = fused(d, S, n, flags)
        fprof, pprof = xf.profile(0), pbf.profile(0)
        tt, _, _ = two_call(d, S, n, flags)
        rows.append({"host_loop_16_threads_s": th, "fused_call_s": tf, "fused_kernels_ms": fms,
                     "fused_summary_count_ms": fprof[3] / 1000.0, "fused_summary_emit_ms": fprof[4] / 1000.0,
                     "fused_mark_ms": pprof[1] / 1000.0, "fused_build_ms": pprof[2] / 1000.0, "two_call": tt})
    col = lambda k: [r[k] for r in rows]
    hh, ff, tt = col("host_loop_16_threads_s"), col("fused_call_s"), [r["two_call"]["call_s"] for r in rows]
    res = {"workload": label, "document": name, "resident_documents": n_docs, "requests": n, "peer_version": v,
           "hello_entries": len(hello), "hello_ranges": sum(len(r) for _n, r in hello), "known_pieces_per_request": prof[0],
           "agent_runs_per_document": int(len(o.export("agent_runs"))), "graph_entries_per_document": int(len(o.export("entries"))),
           "patch_bytes_first": len(got[0]), "patch_bytes_total": len(want), "host_oplogs_loaded": len(distinct), "host_oplog_load_s": load_s, "runs": rows,
           "median_host_loop_16_threads_s": statistics.median(hh), "median_fused_call_s": statistics.median(ff),
           "median_two_call_s": statistics.median(tt),
           "ratio_host_over_fused_median": statistics.median(hh) / statistics.median(ff),
           "ratio_two_call_over_fused_median": statistics.median(tt) / statistics.median(ff),
           "median_summary_kernels_ms": statistics.median([r["fused_summary_count_ms"] + r["fused_summary_emit_ms"] for r in rows]),
           "median_mark_kernel_ms": statistics.median(col("fused_mark_ms")),
           "fused_ahead_of_host_in_every_run": all(b < a for a, b in zip(hh, ff)),
           "fused_behind_host_in_every_run": all(b > a for a, b in zip(hh, ff))}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sync", "bench_sync.json"))
    ap.add_argument("--requests", type=int, default=10000)
    ap.add_argument("--docs", type=int, default=10000, help="resident documents (request i asks document i mod docs)")
    args = ap.parse_args()
    if dt_amd.device_count() < 1:
        raise SystemExit("bench_sync: no HIP device visible (the engine has no CPU fallback)")
    k = args.requests
    n_docs = min(args.docs, k)
    spread = [i % n_docs for i in range(k)]
    results = [
        bench("friendsforever, peer at 0.99 n", "friendsforever", n_docs, spread, lambda o: int(len(o) * 0.99)),
        bench("friendsforever, peer at 0.5 n", "friendsforever", n_docs, spread, lambda o: int(len(o) * 0.5)),
    ]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/bench_sync.py", "host_threads": THREADS, "workloads": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
