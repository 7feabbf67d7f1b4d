#!/usr/bin/env python3
"""What batched blame costs and what it replaces.  Legs, alternating in one process, three runs
each, every run listed:

  plain   a device-staged checkout batch's pass (Batch.run_timed)
  blame   the same documents as a blame batch: its pass (the counting kernels inside it), then the
          first blame read, which sizes the run arena, emits the runs and copies them back
  host    the loop a caller has without it: ListOpLog.xf_operations_lv() per document (a host plan
          and one staged one-document batch per call) plus the Python splice of LVs into a list,
          timed on a sample of the documents and scaled to the batch (the documents of a workload
          are identical and independent; the sample size is in the result)

Workloads: 10,000 friendsforever documents, 64 git-makefile documents, and 256 versions of
friendsforever through DecodeBatch.blame_versions (one call: projection, staging, pass, reads).
The blame kernels' own time, the run and character counts and the bytes of the source-list and
run arenas come from blame_stats().  The spliced list of the host leg is compared with the batch's
runs on the sampled document.  A measurement tool: no threshold is attached.

    python tools/bench_blame.py [--out profiles/blame/bench_blame.json] [--docs 10000]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diamond-types_amd"))
import dt_amd   # noqa: E402


def load(name):
    with open(os.path.join(ROOT, "tests", "golden", "benchmark_data", name + ".dt"), "rb") as f:
        return f.read()


def host_leg(o, calls):
    """The caller's loop of today on one document: transformed positions, then the splice."""
    kind = {}
    for lv, ln, _pos, kf in o.export("ops").reshape(-1, 4):
        for k in range(int(ln)):
            kind[int(lv) + k] = int(kf) & 1
    t0 = time.perf_counter()
    lvs = None
    for _ in range(calls):
        lvs = []
        for lv, x in o.xf_operations_lv():
            if x is None:
                continue
            if kind[lv] == 0:
                lvs.insert(x, lv)
            else:
                del lvs[x]
    return (time.perf_counter() - t0) / calls, lvs


def flat_lvs(runs):
    return [lv + k for lv, n, _a, _s in runs for k in range(n)]


def bench_tip(label, name, n_docs, host_sample, rounds=3):
    data = load(name)
    o = dt_amd.ListOpLog.load_from(data)
    plain = dt_amd.Batch(docs=[data] * n_docs, staging="device")
    blame = dt_amd.Batch(docs=[data] * n_docs, staging="device", blame=True)
    plain.run_timed()
    blame.run_timed()   # warm-up; the legs must agree
    _, want = host_leg(o, 1)
    for i in range(0, n_docs, max(1, n_docs // 8)):
        if flat_lvs(blame.blame(i)) != want or blame.text(i) != plain.text(i):
            raise AssertionError(f"{label}: document {i}'s blame differs from the host splice")
    rows = []
    for _ in range(rounds):
        th, _ = host_leg(o, host_sample)
        tp = plain.run_timed()
        tb = blame.run_timed()
        t0 = time.perf_counter()
        st = blame.blame_stats()   # the first read after the pass: arena sizing, emit, copy back
        rows.append({"host_call_s": th, "host_loop_s": th * n_docs, "plain_pass_ms": tp, "blame_pass_ms": tb,
                     "blame_read_ms": (time.perf_counter() - t0) * 1000.0, "blame_kernels_us": st["kernel_us"],
                     "runs": st["runs"], "chars": st["chars"], "arena_bytes": st["arena_bytes"]})
    col = lambda k: [r[k] for r in rows]
    n_ins = int(sum(int(ln) for _lv, ln, _p, kf in o.export("ops").reshape(-1, 4) if not int(kf) & 1))
    res = {"workload": label, "document": name, "documents": n_docs, "lvs": len(o), "inserted_chars_per_document": n_ins,
           "host_calls_timed_per_run": host_sample, "runs": rows}
    for k in ("host_loop_s", "plain_pass_ms", "blame_pass_ms", "blame_read_ms", "blame_kernels_us"):
        res["median_" + k] = statistics.median(col(k))
    res["arena_bytes_per_inserted_char"] = rows[-1]["arena_bytes"] / float(max(1, n_ins * n_docs))
    res["blame_pass_over_plain_pass_median"] = res["median_blame_pass_ms"] / res["median_plain_pass_ms"]
    res["host_loop_over_blame_pass_and_read_median"] = res["median_host_loop_s"] * 1000.0 / (
        res["median_blame_pass_ms"] + res["median_blame_read_ms"])
    print(json.dumps(res), flush=True)
    return res


def bench_versions(n_versions, rounds=3):
    data = load("friendsforever")
    o = dt_amd.ListOpLog.load_from(data)
    rng = random.Random(5)
    versions = [[rng.randrange(len(o))] for _ in range(n_versions)]
    d = dt_amd.DecodeBatch([data])
    d.run()
    d.blame_versions([0] * n_versions, versions)   # warm-up
    rows = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        out = d.blame_versions([0] * n_versions, versions)
        tb = time.perf_counter() - t0
        t0 = time.perf_counter()
        d.checkout_versions([0] * n_versions, versions)
        rows.append({"blame_versions_s": tb, "checkout_versions_s": time.perf_counter() - t0,
                     "spans": sum(len(s) for _b, s in out)})
    res = {"workload": f"friendsforever, {n_versions} versions through blame_versions", "versions": n_versions, "runs": rows,
           "median_blame_versions_s": statistics.median(r["blame_versions_s"] for r in rows),
           "median_checkout_versions_s": statistics.median(r["checkout_versions_s"] for r in rows)}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blame", "bench_blame.json"))
    ap.add_argument("--docs", type=int, default=10000, help="friendsforever documents")
    ap.add_argument("--host-sample", type=int, default=100, help="host calls timed per run (friendsforever)")
    ap.add_argument("--versions", type=int, default=256)
    args = ap.parse_args()
    if dt_amd.device_count() < 1:
        raise SystemExit("bench_blame: no HIP device visible (the engine has no CPU fallback)")
    results = [
        bench_tip(f"friendsforever x {args.docs}", "friendsforever", args.docs, args.host_sample),
        bench_tip("git-makefile x 64", "git-makefile", 64, 1),
        bench_versions(args.versions),
    ]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/bench_blame.py", "workloads": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
