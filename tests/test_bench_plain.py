"""bench.py's plain run and its options: a plain `--gpus 1 --steps K --warmup W` run times K
passes and prints the headline line alone (`--full` adds the other legs: tests/test_bench_dist.py
runs it); `--dump-outputs DIR` writes the last timed pass's outputs as float .npy files that are
the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FF_LV = 26078        # friendsforever.dt: ListOpLog::len()
FF_TEXT = 21362      # bytes of its checkout
FULL_ONLY = ("e2e", "cold", "encode", "cpu_baseline", "single_doc_latency", "single_doc_table", "cpu_config0")


def _bench(extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--docs", "40"] + extra
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


class _FakeBatch:
    def __init__(self, texts):
        self.texts = texts

    def text(self, i):
        return self.texts[i]


def _fake(n, size):
    texts = [bytes((i + k) % 251 for k in range(size + i % 7)) for i in range(n)]
    res = [dict(status=0, text_len=len(t), text_hash=(0x9E3779B97F4A7C15 * (i + 1)) % 2 ** 64, n_lv=100 + i)
           for i, t in enumerate(texts)]
    return _FakeBatch(texts), res


def test_dump_outputs_layout_and_budget(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_TEXT_BYTES", 5000)
    monkeypatch.setattr(bench, "DUMP_MAX_ROWS", 64)
    batch, res = _fake(100, 300)
    ids = list(range(1000, 1100))
    bench.dump_outputs(batch, res, ids, str(tmp_path / "a"))
    bench.dump_outputs(batch, res, ids, str(tmp_path / "b"))
    for name in ("results", "texts", "text_index"):
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), name
    table = np.load(tmp_path / "a" / "results.npy")
    assert table.shape == (64, 6)
    for row in table:   # exact in float64: ids, lengths and the hash's 32-bit halves
        r = res[int(row[0]) - 1000]
        assert (int(row[2]), int(row[3])) == (r["text_len"], r["n_lv"])
        assert (int(row[4]) << 32) | int(row[5]) == r["text_hash"]
    texts, index = np.load(tmp_path / "a" / "texts.npy"), np.load(tmp_path / "a" / "text_index.npy")
    assert texts.dtype == np.float32 and len(texts) == 5000   # the budget, the last text cut short
    assert [int(x) for x in index[:2, 0]] == [0, 99]
    for i, off, ln in index.astype(np.int64):
        assert bytes(texts[off:off + ln].astype(np.uint8)) == batch.texts[i][:ln]
    assert int(index[-1, 1] + index[-1, 2]) == len(texts)


def test_dump_outputs_small_batch_whole(tmp_path):
    import bench
    batch, res = _fake(3, 10)
    bench.dump_outputs(batch, res, [0, 1, 2], str(tmp_path))
    index = np.load(tmp_path / "text_index.npy").astype(np.int64)
    assert sorted(index[:, 0]) == [0, 1, 2] and np.load(tmp_path / "results.npy").shape == (3, 6)
    assert len(np.load(tmp_path / "texts.npy")) == sum(len(t) for t in batch.texts)


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_same_outputs_twice(tmp_path):
    a = _bench(["--dump-outputs", str(tmp_path / "a")])
    b = _bench(["--dump-outputs", str(tmp_path / "b")])
    assert a["steps"] == 3 and a["warmup"] == 1 and a["full"] is False
    assert a["ms_per_step"] > 0 and a["unit"] == "merged ops/s" and a["higher_is_better"] is True
    assert a["total_merged_ops"] == 40 * FF_LV
    assert a["value"] == pytest.approx(a["total_merged_ops"] / (a["ms_per_step"] / 1e3), rel=1e-9)
    assert not [k for k in FULL_ONLY if k in a]
    size = 0
    for name in ("results", "texts", "text_index"):
        x, y = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), name
        size += x.nbytes
    assert size <= 64_000_000
    table = np.load(tmp_path / "a" / "results.npy")
    assert table.shape == (40, 6) and (table[:, 1] == 0).all() and (table[:, 2] == FF_TEXT).all()
    assert len(np.load(tmp_path / "a" / "texts.npy")) == 40 * FF_TEXT
    golden = os.path.join(ROOT, "tests", "golden", "benchmark_data", "friendsforever_flat.json.gz")
    import gzip
    want = json.load(gzip.open(golden))["endContent"].encode()
    assert bytes(np.load(tmp_path / "a" / "texts.npy")[:FF_TEXT].astype(np.uint8)) == want
