"""bench.py's options around the timed steps: --full (the legs beside the
headline figure, off by default) and --dump-outputs (bench.dump_outputs on
host tensors: the files, their types, the fixed sample)."""
import os

import numpy as np
import torch

import bench

SUMMARY = ("n_traces", "sum_latency", "sum_hops", "sum_err_hops", "n_500", "min_latency", "max_latency")


def _args(monkeypatch, *argv):
    monkeypatch.setattr("sys.argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_has_no_extra_legs(monkeypatch):
    a = _args(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 3)
    a = _args(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d"


def _load(d):
    return {n: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


def test_dump_outputs_small(tmp_path):
    n = 1000
    lat = torch.arange(n, dtype=torch.int64) * 1_000_003 + 5
    hops = torch.arange(n, dtype=torch.int64) % 77
    err = torch.arange(n, dtype=torch.int64) % 3
    recs = torch.stack([lat, hops | (err << 32)], dim=1)
    stats = torch.arange(300, dtype=torch.int64) * 3
    table = torch.arange(40, dtype=torch.int64)
    folded = {k: i + 1 for i, k in enumerate(SUMMARY)}
    bench.dump_outputs(str(tmp_path / "o"), recs, stats, folded, table)
    f = _load(tmp_path / "o")
    assert sorted(f) == ["des_table.npy", "records.npy", "stats.npy", "summary.npy"]
    assert all(v.dtype == np.float64 for v in f.values())
    assert np.array_equal(f["records.npy"], torch.stack([lat, hops, err], dim=1).numpy().astype(np.float64))
    assert np.array_equal(f["stats.npy"], stats.numpy()) and np.array_equal(f["des_table.npy"], table.numpy())
    assert f["summary.npy"].tolist() == [1, 2, 3, 4, 5, 6, 7]
    # no records (--no-records), no table (a walk config)
    bench.dump_outputs(str(tmp_path / "p"), None, stats, folded)
    assert sorted(_load(tmp_path / "p")) == ["stats.npy", "summary.npy"]


def test_dump_outputs_samples_large_outputs(tmp_path):
    n = bench.DUMP_ROWS + 12345
    lat = torch.arange(n, dtype=torch.int64) * 7
    recs = torch.stack([lat, torch.arange(n, dtype=torch.int64) % 100], dim=1)
    stats = torch.arange(bench.DUMP_WORDS + 999, dtype=torch.int64)
    folded = dict.fromkeys(SUMMARY, 0)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), recs, stats, folded)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["records.npy", "records_index.npy", "stats.npy", "stats_index.npy", "summary.npy"]
    assert all(np.array_equal(a[k], b[k]) for k in a)  # the same sample every run
    idx = a["records_index.npy"]
    assert idx.shape == (bench.DUMP_ROWS,) and np.all(np.diff(idx) >= 0) and 0 <= idx[0] and idx[-1] < n
    assert np.array_equal(a["records.npy"][:, 0], idx * 7) and np.array_equal(a["records.npy"][:, 1], idx % 100)
    assert np.array_equal(a["stats.npy"], a["stats_index.npy"]) and a["stats.npy"].shape == (bench.DUMP_WORDS,)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
