"""Timing of the per-window exact percentiles (isim_timeline_quantiles_device,
DESIGN.md §15) against the route a user had without them: copy the 24 B per
trace (arrival + record) to the host and sort per window there.

The inputs are tools/timeline_bench.py's: the config-5 DES batch (2^20 traces,
6 ms mean gap) and the synthetic batch (2^24 traces, arrivals 1 us apart, one
latency of 10 ms), the latter also randomly permuted; windows of 1 s and 1 ms.
At most 65,536 windows are kept, so at 1 ms the DES batch (about 6,300 s long)
puts nearly every record into the "after" row: the case in which one workgroup
selects most of the batch.  Each device call is timed with HIP events (warm-up,
then --reps calls: median, min and max); in the same process the pinned
device-to-host copy of the same 24 B per trace (HIP events) and a numpy
per-window sort on the host (host clock).  Each device table is compared with
the host's before its time is accepted.  The split over the kernels comes from
the profiler's kernel records of --split-calls further calls (not from the
timed ones).  Writes a JSON list (--out).

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
sys.path[:0] = [ROOT, os.path.join(ROOT, "istio-isotope_amd"), os.path.join(ROOT, "tools")]

WINDOWS = {"1s": 10**9, "1ms": 10**6}
Q = (0.5, 0.75, 0.9, 0.99, 0.999)
KERNELS = ("k_tlq_clear", "k_tlq_count", "k_tlq_scan", "k_tlq_scatter", "k_tlq_select")
# -Rpass-analysis=kernel-resource-usage, gfx950
RESOURCES = {"k_tlq_clear": {"vgprs": 6, "lds_bytes": 0, "scratch_bytes": 0, "waves_per_simd": 8},
             "k_tlq_count": {"vgprs": 32, "lds_bytes": 0, "scratch_bytes": 0, "waves_per_simd": 8},
             "k_tlq_scan": {"vgprs": 47, "lds_bytes": 64, "scratch_bytes": 0, "waves_per_simd": 8},
             "k_tlq_scatter": {"vgprs": 36, "lds_bytes": 0, "scratch_bytes": 0, "waves_per_simd": 8},
             "k_tlq_select": {"vgprs": 105, "lds_bytes": 79056, "scratch_bytes": 0, "waves_per_simd": 4}}


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--inputs", default="c5,synthetic,synthetic_permuted")
    ap.add_argument("--reps", type=int, default=20, help="timed device calls per setting")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--split-calls", type=int, default=5, help="further calls whose kernel records give the split")
    ap.add_argument("--shift", type=int, default=0, help="halve every batch this many times (rehearsals)")
    ap.add_argument("--timeout", type=int, default=540, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timeline_quantiles_bench.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def host_quantiles(arr, recs, window, n_windows, ppm):
    """What the host route computes: the same table by numpy sorts (t0 = 0)."""
    import numpy as np
    U = np.uint64
    lat = recs["latency_ns"]
    c = arr + lat
    c[c < arr] = U((1 << 64) - 1)
    rc = (np.minimum(c // U(window), U(n_windows)) + U(1)).astype(np.int64)
    code = (recs["status_err"] >> np.uint32(31)).astype(np.int64)
    rows = n_windows + 2
    out = np.zeros((rows, 3, 1 + len(ppm)), U)

    def fill(key, n_keys, dst):  # dst: [n_keys][1 + n_q] view
        order = np.lexsort((lat, key))
        s = lat[order]
        cnt = np.bincount(key, minlength=n_keys).astype(U)
        start = np.cumsum(cnt) - cnt
        dst[:, 0] = cnt
        has = cnt > 0
        for i, p in enumerate(ppm):
            k = np.maximum((cnt[has] * U(p) + U(999999)) // U(1000000), U(1))
            dst[has, 1 + i] = s[(start[has] + k - U(1)).astype(np.int64)]

    fill(rc, rows, out[:, 0, :])
    by_code = np.zeros((rows * 2, 1 + len(ppm)), U)
    fill(rc * 2 + code, rows * 2, by_code)
    out[:, 1:, :] = by_code.reshape(rows, 2, 1 + len(ppm))
    return out.reshape(-1)


def kernel_split(torch, fn, calls):
    """Mean device time per kernel (ms) over `calls` calls, from the profiler's kernel records."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    split = {}
    for ev in prof.events():
        for k in KERNELS:
            if k in ev.name:
                dur = getattr(ev, "device_time_total", None)
                if dur is None:
                    dur = ev.cuda_time_total
                split[k] = split.get(k, 0.0) + dur / 1e3 / calls
    if not split:
        raise RuntimeError("the profiler recorded none of the kernels")
    return split


def measure(name, args, torch, dev):
    import numpy as np

    import isim
    import timeline_bench as tb
    stream = torch.cuda.current_stream(dev)
    n = max(64, (1 << tb.INPUTS[name][0]) >> args.shift)
    t0 = time.perf_counter()
    h, given, recs, n = tb.make_input(name, n, torch, dev, stream)
    arr = given
    if arr is None:  # the DES batch: the engine's own arrivals
        arr = torch.empty(n, dtype=torch.int64, device=dev)
        awsb = isim.des_arrivals_workspace_bytes(n)
        aws = torch.empty(awsb, dtype=torch.uint8, device=dev)
        isim.des_arrivals_device(h, tb.MEAN_NS, 0, n, d_arrivals=arr.data_ptr(), d_workspace=aws.data_ptr(),
                                 workspace_bytes=awsb, stream=stream.cuda_stream)
        torch.cuda.synchronize()
    print(f"{name}: {n} records ready ({time.perf_counter() - t0:.1f} s)", flush=True)

    def timed(fn, reps):
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return ms

    # the route without the feature: 24 B per trace to the host (pinned), numpy there
    p_rec = torch.empty((n, 2), dtype=torch.int64, pin_memory=True)
    p_arr = torch.empty(n, dtype=torch.int64, pin_memory=True)

    def copy():
        p_rec.copy_(recs, non_blocking=True)
        p_arr.copy_(arr, non_blocking=True)

    copy()
    torch.cuda.synchronize()
    copy_ms = timed(copy, 5)
    h_arr = p_arr.numpy().view(np.uint64)
    h_rec = p_rec.numpy().view(isim.REC_DTYPE).reshape(n)
    span = int(h_arr.max()) + int(h_rec["latency_ns"].max())
    ppm = isim.quantiles.q_to_ppm(Q)

    entries = []
    for wname, window in WINDOWS.items():
        n_windows = max(1, min(isim.native.TL_MAX_WINDOWS, span // window + 1))
        words = isim.timeline_quantiles_out_words(n_windows, len(Q))
        out = torch.empty(words, dtype=torch.int64, device=dev)
        wsb = isim.timeline_quantiles_workspace_bytes(n, n_windows, len(Q))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

        def tlq():
            isim.timeline_quantiles_device(arr.data_ptr(), recs.data_ptr(), n, window, n_windows, 0, Q,
                                           d_out=out.data_ptr(), d_workspace=ws.data_ptr(), workspace_bytes=wsb,
                                           stream=stream.cuda_stream)

        for _ in range(args.warmup):
            tlq()
        dev_ms = timed(tlq, args.reps)
        got = out.cpu().numpy().view(np.uint64)
        t0 = time.perf_counter()
        want = host_quantiles(h_arr, h_rec, window, n_windows, ppm)
        host_ms = (time.perf_counter() - t0) * 1e3
        if not np.array_equal(got, want):
            raise SystemExit(f"{name} {wname}: the device table differs from the host's")
        try:
            split, split_note = kernel_split(torch, tlq, args.split_calls), None
        except Exception as e:  # the split is a report, the times above stand without it
            split, split_note = None, f"{type(e).__name__}: {e}"
        counts = got.reshape(n_windows + 2, 3, 1 + len(Q))[:, 0, 0]
        med = statistics.median(dev_ms)
        e = {"input": name, "why": tb.INPUTS[name][1], "n_records": n, "window": wname, "window_ns": window,
             "n_windows": n_windows, "rows_hit": int((counts > 0).sum()), "longest_row": int(counts.max()),
             "after_row": int(counts[-1]), "table_bytes": words * 8, "workspace_bytes": wsb,
             "device": tb.spread(dev_ms), "kernel_split_ms": split, "kernel_split_note": split_note,
             "slowest_kernel": max(split, key=split.get) if split else None,
             "copy_d2h_pinned": tb.spread(copy_ms), "host_numpy_sort_ms": host_ms,
             "host_ms": statistics.median(copy_ms) + host_ms,
             "host_over_device": (statistics.median(copy_ms) + host_ms) / med,
             "copy_over_device": statistics.median(copy_ms) / med,
             "device_faster_than_copy": bool(med < min(copy_ms))}
        print(json.dumps(e), flush=True)
        entries.append(e)
        del out, ws
    return entries


def worker(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("timeline_quantiles_bench needs a GPU: it measures, it does not fall back")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    entries = []
    for name in args.inputs.split(","):
        entries += measure(name, args, torch, dev)
        torch.cuda.empty_cache()
    from isim import native
    res = {"device": torch.cuda.get_device_name(dev), "library": os.path.basename(native.LIB_PATH),
           "warmup": args.warmup, "quantiles": list(Q),
           "timing": "HIP events around one call; host clock around the numpy sorts; the kernel split from the "
                     "profiler's kernel records of further calls",
           "kernels": RESOURCES, "entries": entries}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


def main():
    args = parse()
    import timeline_bench as tb
    for name in args.inputs.split(","):
        if name not in tb.INPUTS:
            raise SystemExit(f"unknown input {name!r}: one of {', '.join(tb.INPUTS)}")
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
