"""Timing of the device timeline (isim_des_arrivals_device +
isim_timeline_device) against the route a user had without it:
copy the records (and arrival times, had they been exported) to the host and
bin them with numpy there.

Two inputs: a config-5 DES batch (2^20 traces, 6 ms mean gap, its real
arrivals and records) and a synthetic batch (2^24 traces, arrivals 1 us apart,
one latency of 10 ms), the latter also with its traces randomly permuted (every
lane of a wave in another row: no locality).  Per input, windows of 1 s (few
rows), 1 ms (many rows) and 1 ns (at most 65536 windows are kept, so nearly
every time falls into the "after" row).  Each device call is timed with HIP
events (warm-up, then --reps calls: median, min and max); in the same process
the device-to-host copy of the same 24 B per trace into pinned memory (HIP
events) and the numpy binning on the host (host clock).  The device table is
checked against the host's.  Writes a JSON list (--out): the times, the ratio
host / device, and the achieved bytes/s over the one compulsory read of 24 B
per trace.

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

INPUTS = {  # name: (log2 batch, why)
    "c5": (20, "DES batch, 6 ms mean gap: real arrivals, latencies under contention"),
    "synthetic": (24, "arrivals 1 us apart, one latency of 10 ms"),
    "synthetic_permuted": (24, "the same traces in random order: every lane of a wave in another row"),
}
WINDOWS = {"1s": 10**9, "1ms": 10**6, "1ns": 1}
MEAN_NS = 6_000_000


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--inputs", default="c5,synthetic,synthetic_permuted")
    ap.add_argument("--reps", type=int, default=20, help="timed device calls per setting")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=1, help="timed host binnings per setting")
    ap.add_argument("--shift", type=int, default=0, help="halve every batch this many times (rehearsals)")
    ap.add_argument("--timeout", type=int, default=540, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timeline_bench.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def host_timeline(arr, recs, window, n_windows):
    """What the host route computes: the same table by numpy (t0 = 0)."""
    import numpy as np

    from isim import native
    W, U = native.TL_ROW_WORDS, np.uint64
    edges = np.array([round(x * 1e9) for x in __import__("isim").prometheus.DURATION_BUCKETS], np.uint64)
    lat = recs["latency_ns"]
    c = arr + lat
    c[c < arr] = U((1 << 64) - 1)
    ra = (np.minimum(arr // U(window), U(n_windows)) + U(1)).astype(np.int64)
    rc = (np.minimum(c // U(window), U(n_windows)) + U(1)).astype(np.int64)
    code = (recs["status_err"] >> np.uint32(31)).astype(np.int64)
    out = np.zeros((n_windows + 2) * W, U)
    out[native.TL_ARRIVED::W] = np.bincount(ra, minlength=n_windows + 2).astype(U)
    key = rc * W + code
    out += np.bincount(key + native.TL_DONE, minlength=len(out)).astype(U)
    np.add.at(out, key + native.TL_SUM_LAT, lat)
    np.maximum.at(out, key + native.TL_MAX_LAT, lat)
    b = np.searchsorted(edges, lat, side="left").astype(np.int64)
    out += np.bincount(rc * W + native.TL_PROM + code * native.N_PROM + b, minlength=len(out)).astype(U)
    return out


def make_input(name, n, torch, dev, stream):
    """(handler, arrivals tensor or None, records tensor [n, 2] int64, n): c5 serves a DES batch."""
    import numpy as np

    import bench
    import isim
    if name == "c5":
        j, _ = bench.build_graph("c5")
        h = isim.Handler(isim.ServiceGraph.from_json(j), None, isim.SimParams(error_mode=isim.MODE_A))
        d = isim.DesHandler(h, MEAN_NS)
        wsb = d.workspace_bytes(n)
        free = torch.cuda.mem_get_info(dev)[0]
        while n > 4096 and wsb > 0.8 * free:
            n //= 2
            wsb = d.workspace_bytes(n)
        stats = torch.zeros(h.info.stats_words, dtype=torch.int64, device=dev)
        recs = torch.empty((n, 2), dtype=torch.int64, device=dev)
        table = torch.zeros(max(1, d.table_words), dtype=torch.int64, device=dev)
        ws = torch.empty(wsb // 8 + 1, dtype=torch.int64, device=dev)
        for wide in (False, True):
            stats.zero_()
            table.zero_()
            d.serve_device(0, n, recs.data_ptr(), stats.data_ptr(), table.data_ptr(), ws.data_ptr(), wsb,
                           stream.cuda_stream, wide=wide)
            torch.cuda.synchronize()
            if not int(stats[isim.native.ST_DES_RETRY].item()):
                break
        del ws
        torch.cuda.empty_cache()
        return h, None, recs, n
    h = isim.Handler(isim.ServiceGraph.from_json('{"services":[{"name":"a","isEntrypoint":true}]}'), None,
                     isim.SimParams())
    arr = torch.arange(n, dtype=torch.int64, device=dev) * 1000
    recs = torch.zeros((n, 2), dtype=torch.int64, device=dev)
    recs[:, 0] = 10_000_000
    if name == "synthetic_permuted":
        arr = arr[torch.from_numpy(np.random.default_rng(1).permutation(n)).to(dev)].contiguous()
    return h, arr, recs, n


def measure(name, args, torch, dev):
    import numpy as np

    import isim
    stream = torch.cuda.current_stream(dev)
    n = max(64, (1 << INPUTS[name][0]) >> args.shift)
    t0 = time.perf_counter()
    h, given, recs, n = make_input(name, n, torch, dev, stream)
    print(f"{name}: {n} records ready ({time.perf_counter() - t0:.1f} s)", flush=True)
    arr = given if given is not None else torch.empty(n, dtype=torch.int64, device=dev)
    wsb = isim.des_arrivals_workspace_bytes(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

    def arrivals():
        isim.des_arrivals_device(h, MEAN_NS, 0, n, d_arrivals=arr.data_ptr(), d_workspace=ws.data_ptr(),
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

    arr_ms = None
    if given is None:  # the DES batch: its arrivals come from the device call, which is timed too
        for _ in range(args.warmup):
            arrivals()
        arr_ms = timed(arrivals, args.reps)

    # the route without the timeline: 24 B per trace to the host (pinned), numpy there
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

    entries = []
    for wname, window in WINDOWS.items():
        n_windows = max(1, min(isim.native.TL_MAX_WINDOWS, span // window + 1))
        out = torch.zeros(isim.timeline_out_words(n_windows), dtype=torch.int64, device=dev)

        def tl():
            isim.timeline_device(arr.data_ptr(), recs.data_ptr(), n, window, n_windows, d_out=out.data_ptr(),
                                 stream=stream.cuda_stream)

        for _ in range(args.warmup):
            tl()
        tl_ms = timed(tl, args.reps)
        out.zero_()
        tl()
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint64)
        host_ms = []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            want = host_timeline(h_arr, h_rec, window, n_windows)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        if not np.array_equal(got, want):
            raise SystemExit(f"{name} {wname}: the device table differs from the host's")
        dev_ms = statistics.median(tl_ms) + (statistics.median(arr_ms) if arr_ms else 0.0)
        host_total = statistics.median(copy_ms) + statistics.median(host_ms)
        rows_hit = int((got.reshape(-1, isim.native.TL_ROW_WORDS)[:, :3].sum(axis=1) > 0).sum())
        e = {"input": name, "why": INPUTS[name][1], "n_records": n, "window": wname, "window_ns": window,
             "n_windows": n_windows, "rows_hit": rows_hit, "table_bytes": int(out.numel() * 8),
             "timeline": spread(tl_ms), "arrivals": spread(arr_ms) if arr_ms else None,
             "device_ms": dev_ms, "bytes": n * 24, "timeline_gbs": n * 24 / (statistics.median(tl_ms) * 1e-3) / 1e9,
             "copy_d2h_pinned": spread(copy_ms),
             "copy_d2h_pinned_gbs": n * 24 / (statistics.median(copy_ms) * 1e-3) / 1e9,
             "host_numpy": spread(host_ms), "host_ms": host_total,
             "host_over_device": host_total / dev_ms, "copy_over_device": statistics.median(copy_ms) / dev_ms,
             "device_faster_than_copy": bool(dev_ms < min(copy_ms))}
        print(json.dumps(e), flush=True)
        entries.append(e)
    return entries


def worker(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("timeline_bench needs a GPU: it measures, it does not fall back")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    entries = []
    for name in args.inputs.split(","):
        entries += measure(name, args, torch, dev)
    res = {"device": torch.cuda.get_device_name(dev), "warmup": args.warmup,
           "timing": "HIP events around one call; host clock around the numpy binning",
           "kernel": {"name": "k_timeline", "scratch_bytes": 0, "lds_bytes": 37896, "vgprs": 52, "sgprs": 67,
                      "source": "the code object's metadata (hipcc --offload-arch=gfx950 -S)"},
           "entries": entries}
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
