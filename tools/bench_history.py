#!/usr/bin/env python3
"""Checkout at K versions of one resident document: the loop of ListOpLog.checkout(v) (A) against
DecodeBatch.history + one device-staged batch checkout (B), alternating in one process.

Both sides take the host wall clock around work that ends with the texts on the host (a device
sync).  A is the only way to do this without the batched projection, and its code is unchanged by
it.  B's document is decoded on the device once, outside the timing: the resident oplog is the
premise.  Also reported: B's phases (projection call, its two kernels, staging, replay + texts) and
the projection kernels' achieved bytes/s (base SoA read + SoA written per output).

    python tools/bench_history.py [--out profiles/history/bench_history.json]
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diamond-types_amd"))
import dt_amd   # noqa: E402


def versions(n_lv, k, seed):
    rng = random.Random(seed)
    return [sorted(rng.sample(range(n_lv), rng.choice([1, 2, 3]))) for _ in range(k)]


def loop_checkout(full, vs):
    t = time.perf_counter()
    out = [full.checkout(v).content_bytes() for v in vs]
    return time.perf_counter() - t, out


def batch_checkout(d, vs):
    t0 = time.perf_counter()
    h = d.history([0] * len(vs), vs)
    t1 = time.perf_counter()
    for i in range(len(vs)):
        st, _ = h.history_result(i)
        if st:
            raise RuntimeError(f"projection {i}: status {st}")
    prof = h.profile(0)
    nbytes = h.bytes_in() + h.bytes_out()
    ms = h.last_ms
    t2 = time.perf_counter()
    b = h.checkout_batch()
    t3 = time.perf_counter()
    b.run()
    b.sync()
    res = b.results()
    out = []
    for i in range(len(vs)):
        if res[i]["status"]:
            raise RuntimeError(f"checkout {i}: status {res[i]['status']}")
        out.append(b.text(i))
    t4 = time.perf_counter()
    phases = {"history_call_s": t1 - t0, "mark_kernel_ms": prof[1] / 1000.0, "emit_kernel_ms": prof[2] / 1000.0,
              "projection_kernels_ms": ms, "projection_bytes": nbytes,
              "projection_gbps": nbytes / (ms * 1e-3) / 1e9 if ms > 0 else 0.0,
              "staging_s": t3 - t2, "replay_and_texts_s": t4 - t3}
    return t4 - t0, out, phases


def bench(name, k, rounds=3):
    with open(os.path.join(ROOT, "tests", "golden", "benchmark_data", name + ".dt"), "rb") as f:
        data = f.read()
    full = dt_amd.ListOpLog.load_from(data)
    vs = [v for v in versions(len(full), k, 41)]
    d = dt_amd.DecodeBatch([data])
    d.run()
    # warm-up, and the two sides agree
    _, want = loop_checkout(full, vs[:8])
    _, got, _ = batch_checkout(d, vs[:8])
    if want != got:
        raise AssertionError(f"{name}: batched checkout differs from the loop")
    batch_checkout(d, vs)
    rows = []
    for _ in range(rounds):
        a, ta = loop_checkout(full, vs)
        b, tb, ph = batch_checkout(d, vs)
        if ta != tb:
            raise AssertionError(f"{name}: batched checkout differs from the loop")
        rows.append({"loop_s": a, "batch_s": b, "ratio": a / b, **ph})
    return {"document": name, "versions": k, "n_lv": len(full), "alternations": rows,
            "batch_beats_loop_every_time": all(r["batch_s"] < r["loop_s"] for r in rows)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "history", "bench_history.json"))
    a = ap.parse_args()
    if dt_amd.device_count() < 1:
        raise SystemExit("bench_history: no HIP device")
    out = {"friendsforever": bench("friendsforever", 256), "git-makefile": bench("git-makefile", 64)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
