#!/usr/bin/env python3
"""A batch of merges on resident documents: every request takes a branch of a document from `from`
to the tip (iter_xf_operations_from / ListBranch::merge).  Two legs on the same requests,
alternating in one process, every run listed:

  batch   DecodeBatch.xf_operations_from: dtgpu_decode_xf_from, one call for every request
  host    the loop a caller has without it: ListOpLog.xf_operations_lv(from, tip) on host oplogs
          (dtgpu_xf_operations_from: a host plan and one staged one-document batch per call)

The resident documents are decoded on the device once and the host oplogs loaded once, both
outside the timing.  The host leg is timed on a sample of the requests (--host-sample calls; the
requests of a workload are identical and independent, so a call's mean times the request count
is the loop's time; the sample size is in the result).  The batch leg reports the synchronised call
time, the pass's kernel time by stage (dtgpu_merges_profile: projection, prep, plan, replay, LV
translation) and the rest: host staging, and staging's own sizing launches (prep once more and the
count-only planner), which the stage times leave out.  The records of the two legs are compared on
the sampled requests.  A measurement tool: no threshold is attached.

    python tools/bench_merge.py [--out profiles/merge/bench_merge.json] [--requests 10000]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diamond-types_amd"))
import dt_amd   # noqa: E402


def batch_leg(d, docs, frm, tip):
    n = len(docs)
    t0 = time.perf_counter()
    m = d.xf_operations_from(docs, [frm] * n, [tip] * n)
    t = time.perf_counter() - t0
    return t, m


def host_leg(o, frm, tip, calls):
    t0 = time.perf_counter()
    last = None
    for _ in range(calls):
        last = o.xf_operations_lv(frm, tip)
    return (time.perf_counter() - t0) / calls, last


def bench(label, name, n_docs, n_req, frac, host_sample, rounds=3):
    with open(os.path.join(ROOT, "tests", "golden", "benchmark_data", name + ".dt"), "rb") as f:
        data = f.read()
    o = dt_amd.ListOpLog.load_from(data)
    tip = o.local_frontier()
    frm = [int(len(o) * frac)]
    docs = [i % n_docs for i in range(n_req)]
    d = dt_amd.DecodeBatch([data] * n_docs)
    d.run()
    # warm-up at the timed size; the two legs must agree
    _, m = batch_leg(d, docs, frm, tip)
    bad = [i for i in range(n_req) if m.status(i)]
    if bad:
        raise RuntimeError(f"{label}: request {bad[0]} has status {m.status(bad[0])}")
    _, want = host_leg(o, frm, tip, 1)
    for i in range(0, n_req, max(1, n_req // 8)):
        if m.xf_operations_lv(i) != want:
            raise AssertionError(f"{label}: request {i}'s records differ from the host path's")
    n_rec = len(want)
    del m
    rows = []
    for _ in range(rounds):
        th, _ = host_leg(o, frm, tip, host_sample)
        tb, m = batch_leg(d, docs, frm, tip)
        us = m.profile(0)[:5]
        kernels = sum(us) / 1000.0
        rows.append({"host_call_s": th, "host_loop_s": th * n_req, "batch_call_s": tb, "batch_kernels_ms": m.last_ms,
                     "projection_ms": us[0] / 1000.0, "prep_ms": us[1] / 1000.0, "plan_ms": us[2] / 1000.0,
                     "replay_ms": us[3] / 1000.0, "lv_translation_ms": us[4] / 1000.0,
                     "rest_ms": tb * 1000.0 - kernels})
        del m
    col = lambda k: [r[k] for r in rows]
    hh, bb = col("host_loop_s"), col("batch_call_s")
    res = {"workload": label, "document": name, "resident_documents": n_docs, "requests": n_req, "from": frm, "lvs": len(o),
           "graph_entries_per_document": int(len(o.export("entries"))), "records_per_request": n_rec,
           "host_calls_timed_per_run": host_sample, "runs": rows,
           "median_host_loop_s": statistics.median(hh), "median_batch_call_s": statistics.median(bb),
           "ratio_host_over_batch_median": statistics.median(hh) / statistics.median(bb)}
    for k in ("batch_kernels_ms", "projection_ms", "prep_ms", "plan_ms", "replay_ms", "lv_translation_ms", "rest_ms"):
        res["median_" + k] = statistics.median(col(k))
    res["batch_ahead_of_host_in_every_run"] = all(b < a for a, b in zip(hh, bb))
    res["batch_behind_host_in_every_run"] = all(b > a for a, b in zip(hh, bb))
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge", "bench_merge.json"))
    ap.add_argument("--requests", type=int, default=10000, help="friendsforever requests, one resident document each")
    ap.add_argument("--host-sample", type=int, default=100, help="host calls timed per run (friendsforever)")
    args = ap.parse_args()
    if dt_amd.device_count() < 1:
        raise SystemExit("bench_merge: no HIP device visible (the engine has no CPU fallback)")
    k = args.requests
    results = [
        bench("friendsforever, from 0.99 n", "friendsforever", k, k, 0.99, args.host_sample),
        bench("friendsforever, from 0.5 n", "friendsforever", k, k, 0.5, args.host_sample),
        bench("git-makefile, 64 requests, from 0.5 n", "git-makefile", 64, 64, 0.5, 4),
    ]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/bench_merge.py", "workloads": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
