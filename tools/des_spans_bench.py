"""Timing of the DES span tap (isim_serve_des_spans_device) on a
config-5p DES step of 2^19 traces at bench.py's own mean gap: the same call
with a NULL tap, which is isim_serve_des_device, and with the tap at the
batch's p99.9 (its spans and the wait table).  The NULL-tap call in the same
process is the yardstick; the tap's own kernels and its two read-backs are the
difference of the medians (no ratio is fixed in advance).

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
    ap.add_argument("--q-ppm", type=int, default=999000)
    ap.add_argument("--max-traces", type=int, default=1024)
    ap.add_argument("--cap-spans", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=400, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "des_spans_bench.json"))
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

    t_null = timed(lambda: call(None))
    t_tap = timed(lambda: call(tap))
    word = info.cpu().numpy().view(np.uint64)
    out = {"device": torch.cuda.get_device_name(0), "graph": "bench.build_graph('c5p')", "n_traces": n,
           "mean_interarrival_ns": a.mean_ns, "q_ppm": a.q_ppm, "matches": int(word[native.DES_SPAN_MATCHES]),
           "traces_written": int(word[native.SPAN_WRITTEN]), "spans": int(word[native.SPAN_TOTAL]),
           "span_bytes": int(word[native.SPAN_TOTAL]) * 64, "items": d.last_batch()["items"],
           "null_tap": t_null, "tap_p999": t_tap,
           "tap_overhead_ms": t_tap["median_ms"] - t_null["median_ms"],
           "tap_overhead_pct": 100.0 * (t_tap["median_ms"] - t_null["median_ms"]) / t_null["median_ms"]}
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
        print(f"des_spans_bench: the measuring process passed its limit of {a.timeout} s", file=sys.stderr)
        rc = 124
    sys.exit(rc)


if __name__ == "__main__":
    main()
