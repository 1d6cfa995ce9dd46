"""Timing of DES worker pools (isim_des_workers_set) on a
config-5p DES step of 2^19 traces at bench.py's own mean gap, one
isim_serve_des_device call each:

  (a) workers never set;
  (b) all workers set to 1 — the same launches as (a): any difference beyond the
      spread of (a)'s own calls is a bug, not a cost;
  (c) 4 workers on every service;
  (d) 4 workers on the busiest service only (the largest hold total of (a)).

For (c) and (d) the added time is reported next to the batch's wait totals;
no figure is fixed in advance.

Each call is timed with HIP events (--warmup calls, then --reps: median, min
and max).  The parent process never opens the GPU: it starts the measuring
process under a time limit (--timeout) and reports its exit status.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "istio-isotope_amd")]


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2n", type=int, default=19, help="traces of the DES step")
    ap.add_argument("--mean-ns", type=int, default=6_000_000, help="mean inter-arrival gap (bench.py's for c5p)")
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=400, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "des_workers_bench.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def worker(a):
    import numpy as np
    import torch

    import bench
    import isim
    from isim import native

    dev = torch.device("cuda", 0)
    torch.cuda.init()
    stream = torch.cuda.current_stream(dev).cuda_stream
    j, _ = bench.build_graph("c5p")
    h = isim.Handler(isim.ServiceGraph.from_json(j), None, isim.SimParams())
    d = isim.DesHandler(h, a.mean_ns)
    assert d.info.items == 1 and d.info.cyclic == 0
    n = 1 << a.log2n
    ns = int(h.info.n_services)

    def i64(words):
        return torch.zeros(max(1, words), dtype=torch.int64, device=dev)

    ws = torch.empty(d.workspace_bytes(n) + 8, dtype=torch.uint8, device=dev)
    recs, stats, table = i64(2 * n), i64(len(h.new_stats())), i64(d.table_words)

    def call():
        d.serve_device(1 << 31, n, recs.data_ptr(), stats.data_ptr(), table.data_ptr(), ws.data_ptr(), ws.numel(),
                       stream)

    def timed():
        for _ in range(a.warmup):
            call()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        # the figures of one batch: the tables start from zero
        stats.zero_()
        table.zero_()
        call()
        torch.cuda.synchronize()
        rows = d.fold(table.cpu().numpy().view(np.uint64))
        r = recs.cpu().numpy().view(isim.REC_DTYPE)
        out = spread(ms)
        out.update(sum_wait_ns=int(rows[:, native.DES_SUM_WAIT].sum()), max_wait_ns=int(rows[:, native.DES_MAX_WAIT].max()),
                   sum_latency_ns=int(r["latency_ns"].sum(dtype=np.uint64)), syncs=d.last_batch()["syncs"])
        return out, rows, r.copy()

    t_a, rows_a, recs_a = timed()
    d.workers = 1
    t_b, rows_b, recs_b = timed()
    assert np.array_equal(rows_a, rows_b) and np.array_equal(recs_a, recs_b)
    d.workers = a.workers
    t_c, _, _ = timed()
    busiest = int(np.argmax(rows_a[:, native.DES_SUM_HOLD]))
    w = np.ones(ns, np.uint32)
    w[busiest] = a.workers
    d.workers = w
    t_d, _, _ = timed()
    out = {"device": torch.cuda.get_device_name(0), "graph": "bench.build_graph('c5p')", "n_traces": n,
           "mean_interarrival_ns": a.mean_ns, "workers": a.workers, "items": d.last_batch()["items"],
           "busiest_service": busiest, "never_set": t_a, "all_one": t_b, "all_pooled": t_c, "busiest_pooled": t_d,
           "all_one_minus_never_set_ms": t_b["median_ms"] - t_a["median_ms"],
           "never_set_spread_ms": t_a["max_ms"] - t_a["min_ms"],
           "all_pooled_added_ms": t_c["median_ms"] - t_a["median_ms"],
           "busiest_pooled_added_ms": t_d["median_ms"] - t_a["median_ms"]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def main():
    a = parse()
    if a.worker:
        return worker(a)
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"] + sys.argv[1:],
                            timeout=a.timeout).returncode
    except subprocess.TimeoutExpired:
        print(f"des_workers_bench: the measuring process passed its limit of {a.timeout} s", file=sys.stderr)
        rc = 124
    sys.exit(rc)


if __name__ == "__main__":
    main()
