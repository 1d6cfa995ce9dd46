"""Timing of the DES critical-path fold (isim_des_critical_path_device, DESIGN.md
§22) on §21's batch: a config-5p DES step of 2^19 traces at bench.py's own mean
gap with the tap at the batch's p99.9; the fold runs over the spans that tap
wrote.  Two yardsticks in the same process: the tap call itself, and the way
without the device fold, a pinned device-to-host copy of the spans followed by
isim_des_critical_path_host (wall clock: it is host work).  The device and host
tables are asserted equal.  No ratio is fixed in advance.

The device calls are timed with HIP events (--warmup calls, then --reps: median,
min and max).  The parent process never opens the GPU: it starts the measuring
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
    ap.add_argument("--q-ppm", type=int, default=999000)
    ap.add_argument("--max-traces", type=int, default=1024)
    ap.add_argument("--cap-spans", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=400, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "des_critical_path_bench.json"))
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
    from isim.des_spans import make_tap

    dev = torch.device("cuda", 0)
    torch.cuda.init()
    stream = torch.cuda.current_stream(dev).cuda_stream
    j, _ = bench.build_graph("c5p")
    h = isim.Handler(isim.ServiceGraph.from_json(j), None, isim.SimParams())
    d = isim.DesHandler(h, a.mean_ns)
    assert d.info.items == 1
    n = 1 << a.log2n

    def i64(words):
        return torch.zeros(max(1, words), dtype=torch.int64, device=dev)

    ws = torch.empty(d.workspace_bytes(n) + 8, dtype=torch.uint8, device=dev)
    recs, stats, table = i64(2 * n), i64(len(h.new_stats())), i64(d.table_words)
    ids, off, info = i64(a.max_traces), i64(a.max_traces + 1), i64(native.DES_SPAN_INFO_WORDS)
    spans = torch.empty(a.cap_spans * 64, dtype=torch.uint8, device=dev)
    wait = i64((h.info.n_services + 1) * native.DW_ROW_WORDS)
    tap = make_tap(0, a.q_ppm, native.Q_ALL, a.max_traces, a.cap_spans, ids.data_ptr(), off.data_ptr(),
                   spans.data_ptr(), info.data_ptr(), wait.data_ptr())

    def call(t):
        d.serve_spans_device(1 << 31, n, recs.data_ptr(), stats.data_ptr(), table.data_ptr(), ws.data_ptr(),
                             ws.numel(), t, stream)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return spread(ms)

    import time

    from isim.des_spans import (critical_path_table_words, critical_path_workspace_bytes, des_critical_path_device,
                                des_critical_path_host)

    t_tap = timed(lambda: call(tap))
    word = info.cpu().numpy().view(np.uint64)
    written, total = int(word[native.SPAN_WRITTEN]), int(word[native.SPAN_TOTAL])
    assert written > 0 and total <= a.cap_spans
    words = critical_path_table_words(h)
    cws_bytes = critical_path_workspace_bytes(h, a.cap_spans)
    cws = torch.empty(cws_bytes, dtype=torch.uint8, device=dev)
    cpt, tw = i64(words), i64(a.max_traces)

    def fold():
        des_critical_path_device(h, off.data_ptr(), spans.data_ptr(), a.cap_spans, info.data_ptr(), a.max_traces,
                                 cpt.data_ptr(), tw.data_ptr(), cws.data_ptr(), cws_bytes, stream)

    # the spans before any fold, for the host's way; the fold only ORs a bit into them, so it repeats
    clean = spans[:total * 64].cpu().numpy().view(isim.DES_SPAN_DTYPE).copy()
    h_off = off.cpu().numpy().view(np.uint64)[:written + 1].copy()
    t_fold = timed(fold)
    cpt.zero_()
    fold()
    torch.cuda.synchronize()
    d_table = cpt.cpu().numpy().view(np.uint64).copy()
    d_wait = tw.cpu().numpy().view(np.uint64)[:written].copy()
    d_spans = spans[:total * 64].cpu().numpy().view(isim.DES_SPAN_DTYPE)

    pinned = torch.empty(total * 64, dtype=torch.uint8).pin_memory()
    host_ms = []
    for r in range(a.warmup + a.reps):
        spans[:total * 64].copy_(torch.from_numpy(clean.view(np.uint8)))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pinned.copy_(spans[:total * 64], non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        hs = pinned.numpy().view(isim.DES_SPAN_DTYPE)
        h_table, h_wait = np.zeros(words, np.uint64), np.zeros(written, np.uint64)
        des_critical_path_host(h, h_off, written, hs, h_table, h_wait)
        t2 = time.perf_counter()
        if r >= a.warmup:
            host_ms.append((1e3 * (t2 - t0), 1e3 * (t1 - t0)))
    assert np.array_equal(h_table, d_table) and np.array_equal(h_wait, d_wait) and np.array_equal(hs, d_spans)
    t = d_table.reshape(-1, native.DCP_ROW_WORDS)
    ns = h.info.n_services
    parts = {k: int(t[:ns, w].sum(dtype=np.uint64)) for k, w in (("wait_ns", native.DCP_WAIT_NS),
                                                                   ("self_ns", native.DCP_SELF_NS),
                                                                   ("hop_ns", native.DCP_HOP_NS))}
    latency = int(t[ns, native.DCP_H_SUM_LATENCY])
    assert sum(parts.values()) == latency and int(t[ns, native.DCP_H_REFUSED]) == 0
    t_host = spread([x[0] for x in host_ms])
    out = {"device": torch.cuda.get_device_name(0), "graph": "bench.build_graph('c5p')", "n_traces": n,
           "mean_interarrival_ns": a.mean_ns, "q_ppm": a.q_ppm, "traces": written, "spans": total,
           "critical_spans": int(t[ns, native.DCP_H_CRITICAL]), "sum_latency_ns": latency, **parts,
           "tap_p999": t_tap, "fold_device": t_fold, "copy_and_host_fold": t_host,
           "copy_only_ms": statistics.median(x[1] for x in host_ms),
           "fold_ns_per_span": 1e6 * t_fold["median_ms"] / total,
           "fold_over_tap_call": t_fold["median_ms"] / t_tap["median_ms"],
           "fold_over_copy_and_host_fold": t_fold["median_ms"] / t_host["median_ms"],
           "tables_equal": True}
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
        print(f"des_critical_path_bench: the measuring process passed its limit of {a.timeout} s", file=sys.stderr)
        rc = 124
    sys.exit(rc)


if __name__ == "__main__":
    main()
