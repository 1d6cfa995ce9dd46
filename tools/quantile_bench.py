"""Timing of the exact device percentiles (isim_latency_quantiles_device,
DESIGN.md §13) against the route a user had without them: copy the records to
the host and np.partition there.

Three inputs, each served once with records on the GPU: config 3 in mode A
(2^24 traces, ONE latency in every record: the contended case of the LDS
histogram), config 3 at probability 50 (c3p, 2^22, spread latencies) and a
config-5 DES batch (2^20, spread latencies under contention).  Per input the
select is timed with HIP events (warm-up, then --reps calls: median, min and
max), then in the same process the device-to-host copy of the same records
(into pinned memory, HIP events; into pageable memory, host clock around a
synchronising copy) and np.partition per class on the host.  The select's
result is checked against the host's.  Writes a JSON list (--out), one entry
per input: the times, the digit passes actually run, the reads of the
records (the count pass + the digit passes), bytes = reads x n x 16 and the
resulting GB/s.

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

INPUTS = {  # name: (bench.py config, log2 batch, why)
    "c3": ("c3", 24, "mode A static walk: one latency in every record (the contended case)"),
    "c3p": ("c3p", 22, "probability 50 on every call: spread latencies"),
    "c5": ("c5", 20, "DES batch, 6 ms mean gap: spread latencies under contention"),
}


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--inputs", default="c3,c3p,c5")
    ap.add_argument("--reps", type=int, default=20, help="timed select calls per input")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3, help="timed host copies / partitions per input")
    ap.add_argument("--shift", type=int, default=0, help="halve every batch this many times (rehearsals)")
    ap.add_argument("--timeout", type=int, default=540, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantile_bench.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def serve_records(name, n, torch, dev, stream):
    """One batch of n traces with records on the device: (records tensor [n, 2] int64, actual n)."""
    import bench
    import isim
    cfg = INPUTS[name][0]
    j, _ = bench.build_graph(cfg)
    h = isim.Handler(isim.ServiceGraph.from_json(j), None, isim.SimParams(error_mode=isim.MODE_A))
    stats = torch.zeros(h.info.stats_words, dtype=torch.int64, device=dev)
    if cfg != "c5":
        recs = torch.empty((n, 2), dtype=torch.int64, device=dev)
        h.serve_device(0, n, recs.data_ptr(), stats.data_ptr(), stream.cuda_stream)
        torch.cuda.synchronize()
        return recs, n
    d = isim.DesHandler(h, 6_000_000)
    wsb = d.workspace_bytes(n)
    free = torch.cuda.mem_get_info(dev)[0]
    while n > 4096 and wsb > 0.8 * free:  # a device with less free HBM: the largest halving that fits
        n //= 2
        wsb = d.workspace_bytes(n)
    recs = torch.empty((n, 2), dtype=torch.int64, device=dev)
    table = torch.zeros(max(1, d.table_words), dtype=torch.int64, device=dev)
    ws = torch.empty(wsb // 8 + 1, dtype=torch.int64, device=dev)
    d.serve_device(0, n, recs.data_ptr(), stats.data_ptr(), table.data_ptr(), ws.data_ptr(), wsb, stream.cuda_stream)
    torch.cuda.synchronize()
    if int(stats[isim.native.ST_DES_RETRY].item()):  # a latency past 2^31 ns: 64-bit rows
        stats.zero_()
        table.zero_()
        d.serve_device(0, n, recs.data_ptr(), stats.data_ptr(), table.data_ptr(), ws.data_ptr(), wsb,
                       stream.cuda_stream, wide=True)
        torch.cuda.synchronize()
    del ws
    torch.cuda.empty_cache()
    return recs, n


def host_quantiles(host, ppm):
    """What the host route computes: per class the count and the nearest-rank values by np.partition."""
    import numpy as np
    lat, is500 = host["latency_ns"], (host["status_err"] >> np.uint32(31)).astype(bool)
    out = np.zeros((3, 1 + len(ppm)), np.uint64)
    for c, x in enumerate((lat, lat[~is500], lat[is500])):
        out[c, 0] = len(x)
        if len(x):
            ks = [max(1, -((-p * len(x)) // 10**6)) - 1 for p in ppm]
            part = np.partition(x, sorted(set(ks)))
            out[c, 1:] = [part[k] for k in ks]
    return out


def measure(name, args, torch, dev):
    import numpy as np

    import isim
    from isim import quantiles
    stream = torch.cuda.current_stream(dev)
    n = max(64, (1 << INPUTS[name][1]) >> args.shift)
    t0 = time.perf_counter()
    recs, n = serve_records(name, n, torch, dev, stream)
    print(f"{name}: {n} records served ({time.perf_counter() - t0:.1f} s with the graph build)", flush=True)
    q = isim.DEFAULT_Q
    ppm = quantiles.q_to_ppm(q)
    wsb = isim.quantiles_workspace_bytes(len(q))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    out = torch.zeros(isim.quantiles_out_words(len(q)), dtype=torch.int64, device=dev)

    def select():
        isim.latency_quantiles_device(recs.data_ptr(), n, q, d_out=out.data_ptr(), d_workspace=ws.data_ptr(),
                                      workspace_bytes=wsb, stream=stream.cuda_stream)

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

    for _ in range(args.warmup):
        select()
    torch.cuda.synchronize()
    sel = timed(select, args.reps)
    got = out.cpu().numpy().view(np.uint64).reshape(3, 1 + len(q))

    # the route without the select: records to the host, np.partition there
    pinned = torch.empty((n, 2), dtype=torch.int64, pin_memory=True)
    pinned.copy_(recs, non_blocking=True)
    torch.cuda.synchronize()
    copy_pinned = timed(lambda: pinned.copy_(recs, non_blocking=True), max(args.host_reps, 5))
    copy_pageable, part = [], []
    for _ in range(args.host_reps):
        t0 = time.perf_counter()
        host = recs.cpu()
        copy_pageable.append((time.perf_counter() - t0) * 1e3)
    host = host.numpy().view(isim.REC_DTYPE).reshape(n)
    for _ in range(args.host_reps):
        t0 = time.perf_counter()
        want = host_quantiles(host, ppm)
        part.append((time.perf_counter() - t0) * 1e3)
    if not np.array_equal(got, want):
        raise SystemExit(f"{name}: device quantiles {got.tolist()} differ from the host's {want.tolist()}")

    top = int(host["latency_ns"].max())
    digit_passes = (top.bit_length() + 7) // 8
    reads = 1 + digit_passes
    nbytes = reads * n * 16
    e = {"input": name, "why": INPUTS[name][2], "n_records": n, "q": list(q),
         "distinct_latencies": int(len(np.unique(host["latency_ns"]))),
         "count_500": int(want[2, 0]), "p50_ns": int(want[0, 1]), "p999_ns": int(want[0, 5]),
         "select": spread(sel), "digit_passes": digit_passes, "record_reads": reads, "bytes": nbytes,
         "select_gbs": nbytes / (statistics.median(sel) * 1e-3) / 1e9,
         "copy_d2h_pinned": spread(copy_pinned),
         "copy_d2h_pinned_gbs": n * 16 / (statistics.median(copy_pinned) * 1e-3) / 1e9,
         "copy_d2h_pageable": spread(copy_pageable), "host_partition": spread(part),
         "copy_over_select": statistics.median(copy_pinned) / statistics.median(sel),
         "select_faster_than_copy": bool(max(sel) < min(copy_pinned))}
    print(json.dumps(e), flush=True)
    return e


def worker(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("quantile_bench needs a GPU: it measures, it does not fall back")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from isim import native
    res = {"device": torch.cuda.get_device_name(dev), "library": os.path.basename(native.LIB_PATH), "warmup": args.warmup,
           "timing": "HIP events around one call; host clock around the pageable copy and np.partition",
           "entries": [measure(name, args, torch, dev) for name in args.inputs.split(",")]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


def main():
    args = parse()
    for name in args.inputs.split(","):
        if name not in INPUTS:
            raise SystemExit(f"unknown input {name!r}: one of {', '.join(INPUTS)}")
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
