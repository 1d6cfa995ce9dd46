"""Timing of the closed-loop arrivals (isim_closed_loop_device)
over the records of a served config-3 batch, at 1, 4, 64, 4096 and 65,536
connections, at qps "max" (period 0) and paced (a period of 1.25 mean
latencies per connection), against two things in the same process:

  * isim_des_arrivals_device at the same n: existing code of the same shape,
    a chunked scan that writes 8 B per trace;
  * the host route: the records copied to pinned host memory and the
    per-connection closed form in numpy (F_k = P_k + max(F_in, max_j (s_j - P_{j-1}))).

Each device call is timed with HIP events (--warmup calls, then --reps: median,
min and max); the host route with the host clock (--host-reps).  The design
moves 40 B per request (the 16-byte records read twice, 8 B written): the JSON
(--out) reports the achieved bytes per second against that, and every C at
which the call costs more than the device-to-host copy alone.

The parent process never opens the GPU: it starts the measuring process under
a time limit (--timeout) and reports its exit status.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "istio-isotope_amd")]

CONNECTIONS = (1, 4, 64, 4096, 65536)
BYTES_PER_REQUEST = 40


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2n", type=int, default=24, help="records of the batch")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=540, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closed_loop_bench.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def closed_form(np, C, p, lat):
    """The arrivals of a run from zeros over lat (u64, nothing saturates), per connection in numpy."""
    n = len(lat)
    rows = -(-n // C)
    L = np.zeros(rows * C, np.int64)
    L[:n] = lat
    L = L.reshape(rows, C)
    s = (np.arange(rows, dtype=np.int64) * p)[:, None]
    P = np.cumsum(L, axis=0)
    F = P + np.maximum(0, np.maximum.accumulate(s - (P - L), axis=0))
    A = np.maximum(np.vstack([np.zeros((1, C), np.int64), F[:-1]]), s)
    return A.reshape(-1)[:n]


def worker(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("closed_loop_bench needs a GPU: it measures, it does not fall back")
    import bench
    import isim
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return ms

    n = 1 << args.log2n
    j, _ = bench.build_graph("c3")
    h = isim.Handler(isim.ServiceGraph.from_json(j), None, isim.SimParams(error_mode=isim.MODE_A))
    recs = torch.empty((n, 2), dtype=torch.int64, device=dev)
    stats = torch.zeros(h.stats_words, dtype=torch.int64, device=dev)
    h.serve_device(0, n, recs.data_ptr(), stats.data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize()
    mean_lat = int(stats[isim.native.ST_SUM_LATENCY].item()) // n
    arr = torch.empty(n, dtype=torch.int64, device=dev)
    info = torch.empty(4, dtype=torch.int64, device=dev)
    wsb = max([isim.closed_loop_workspace_bytes(n, c) for c in CONNECTIONS] + [isim.des_arrivals_workspace_bytes(n)])
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    base = timed(lambda: isim.des_arrivals_device(h, 6_000_000, 0, n, d_arrivals=arr.data_ptr(),
                                                  d_workspace=ws.data_ptr(), workspace_bytes=wsb,
                                                  stream=stream.cuda_stream))
    pinned = torch.empty((n, 2), dtype=torch.int64).pin_memory()
    copy_ms = timed(lambda: pinned.copy_(recs, non_blocking=True))
    entries = []
    for C in CONNECTIONS:
        free = torch.zeros(C, dtype=torch.int64, device=dev)
        for p in (0, mean_lat * 5 // 4):
            cl = isim.ClosedLoop(C, period_ns=p)

            def call():
                free.zero_()
                cl.arrivals_device(recs.data_ptr(), n, 0, d_free_at=free.data_ptr(), d_arrivals=arr.data_ptr(),
                                   d_info=info.data_ptr(), d_workspace=ws.data_ptr(), workspace_bytes=wsb,
                                   stream=stream.cuda_stream)

            ms = timed(call)
            torch.cuda.synchronize()
            got = arr.cpu().numpy()
            host_ms = []
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                pinned.copy_(recs, non_blocking=True)
                torch.cuda.synchronize()
                want = closed_form(np, C, p, pinned.numpy()[:, 0])
                host_ms.append((time.perf_counter() - t0) * 1e3)
            med = statistics.median(ms)
            e = {"n": n, "connections": C, "period_ns": p, "device": spread(ms), "des_arrivals": spread(base),
                 "device_over_des_arrivals": med / statistics.median(base),
                 "host_copy": spread(copy_ms), "host_copy_and_numpy": spread(host_ms),
                 "device_over_host_copy": med / statistics.median(copy_ms),
                 "costs_more_than_host_copy": bool(med > statistics.median(copy_ms)),
                 "achieved_GBps_of_40B_per_request": BYTES_PER_REQUEST * n / (med * 1e-3) / 1e9,
                 "equals_numpy_closed_form": bool(np.array_equal(got, want)),
                 "makespan_ns": int(info[0].item()), "late": int(info[2].item())}
            print(json.dumps(e), flush=True)
            entries.append(e)
    res = {"device": torch.cuda.get_device_name(dev), "warmup": args.warmup,
           "timing": "HIP events around one call (the host route: host clock around copy, synchronise and numpy)",
           "graph": "c3", "mean_latency_ns": mean_lat, "bytes_per_request": BYTES_PER_REQUEST, "entries": entries}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


def main():
    args = parse()
    if args.worker:
        return worker(args)
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"] + sys.argv[1:],
                            timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit(f"the measuring process passed {args.timeout} s and was stopped")
    sys.exit(rc)


if __name__ == "__main__":
    main()
