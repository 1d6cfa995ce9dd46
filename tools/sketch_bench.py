"""Timing of the mergeable latency sketch (isim_latency_sketch_device,
isim_timeline_sketch_device) against two baselines measured in
the same process on the same batch: the exact calls (isim_latency_quantiles_device,
isim_timeline_quantiles_device) and the pinned device-to-host copy of the
same bytes (16 B per trace, 24 B with the arrivals).

Whole batch: tools/quantile_bench.py's three served batches (c3: one latency
in every record, c3p, the c5 DES batch).  Per window: the settings of
tools/timeline_quantiles_bench.py (the c5 DES batch and the synthetic batch,
the latter also randomly permuted; windows of 1 s and 1 ms, at most 65,536).
Both at sub_bits 3 and 7.  Each call is timed with HIP events (warm-up, then
--reps calls into a table that keeps accumulating: median, min and max).  Each
device table is compared with the host's (the bucket rule restated in numpy,
the table cleared and filled once) before its time is accepted.  Writes a
JSON list (--out).

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
SUB_BITS = (3, 7)
# COPIED by hand from `hipcc -Rpass-analysis=kernel-resource-usage` on csrc/sketch.hip (gfx950, the Makefile's
# flags) as DESIGN.md §16 lists them; not derived at run time: after an edit of a kernel, recompile and update
# both.  The output file repeats this under "kernels_note".
RESOURCES_NOTE = ("copied from -Rpass-analysis=kernel-resource-usage at the time the tool was written, "
                  "not measured by this run")
RESOURCES = {"k_sketch": {"vgprs": 24, "lds_bytes": 59392, "scratch_bytes": 0, "waves_per_simd": 4},
             "k_timeline_sketch": {"vgprs": 46, "lds_bytes": 59396, "scratch_bytes": 0, "waves_per_simd": 4}}


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch-inputs", default="c3,c3p,c5", help="whole-batch inputs (quantile_bench's); '' for none")
    ap.add_argument("--window-inputs", default="c5,synthetic,synthetic_permuted",
                    help="per-window inputs (timeline_quantiles_bench's); '' for none")
    ap.add_argument("--reps", type=int, default=20, help="timed device calls per setting")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shift", type=int, default=0, help="halve every batch this many times (rehearsals)")
    ap.add_argument("--timeout", type=int, default=900, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sketch_bench.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def names(arg):
    return [x for x in arg.split(",") if x]


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def bucket_np(s, v):
    """The bucket rule (isim.h) over a u64 array: shifts and compares only."""
    import numpy as np
    U = np.uint64
    x = v.copy()
    bl = np.zeros(v.shape, np.int64)
    for sh in (32, 16, 8, 4, 2, 1):
        m = x >= (U(1) << U(sh))
        bl += m * sh
        x = np.where(m, x >> U(sh), x)
    bl += x > 0
    shift = np.maximum(bl - (s + 1), 0)
    return (shift << s) + (v >> shift.astype(U)).astype(np.int64)


def same_table(np, table, keys):
    """The device table (u64 words) holds exactly the counts of the host's keys."""
    want_k, want_c = np.unique(keys, return_counts=True)
    got_k = np.flatnonzero(table)
    return np.array_equal(got_k, want_k) and np.array_equal(table[got_k], want_c.astype(np.uint64))


def timer(torch, stream):
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
    return timed


def measure_batch(name, args, torch, dev):
    import numpy as np

    import isim
    import quantile_bench as qb
    stream = torch.cuda.current_stream(dev)
    timed = timer(torch, stream)
    n = max(64, (1 << qb.INPUTS[name][1]) >> args.shift)
    t0 = time.perf_counter()
    recs, n = qb.serve_records(name, n, torch, dev, stream)
    print(f"{name}: {n} records served ({time.perf_counter() - t0:.1f} s with the graph build)", flush=True)

    # baseline 1: the exact select, unchanged
    q = isim.DEFAULT_Q
    wsb = isim.quantiles_workspace_bytes(len(q))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    qout = torch.zeros(isim.quantiles_out_words(len(q)), dtype=torch.int64, device=dev)

    def select():
        isim.latency_quantiles_device(recs.data_ptr(), n, q, d_out=qout.data_ptr(), d_workspace=ws.data_ptr(),
                                      workspace_bytes=wsb, stream=stream.cuda_stream)

    for _ in range(args.warmup):
        select()
    sel = timed(select, args.reps)
    exact = isim.quantiles.decode_quantiles(qout.cpu().numpy().view(np.uint64), q)
    # baseline 2: the pinned copy of the same bytes
    pinned = torch.empty((n, 2), dtype=torch.int64, pin_memory=True)
    pinned.copy_(recs, non_blocking=True)
    torch.cuda.synchronize()
    copy_ms = timed(lambda: pinned.copy_(recs, non_blocking=True), 5)
    host = pinned.numpy().view(isim.REC_DTYPE).reshape(n)
    code = (host["status_err"] >> np.uint32(31)).astype(np.int64)

    entries = []
    for s in SUB_BITS:
        table = torch.zeros(isim.sketch_words(s), dtype=torch.int64, device=dev)

        def sketch():
            isim.latency_sketch_device(recs.data_ptr(), n, s, d_table=table.data_ptr(), stream=stream.cuda_stream)

        sketch()
        got = table.cpu().numpy().view(np.uint64)
        if not same_table(np, got, code * isim.sketch_bins(s) + bucket_np(s, host["latency_ns"])):
            raise SystemExit(f"{name} s={s}: the device table differs from the host's")
        brackets = isim.sketch_quantiles(s, got, q)
        for cls in brackets:
            for f in q:
                lo, hi = brackets[cls]["q"][f]
                if not lo <= exact[cls]["q"][f] <= hi:
                    raise SystemExit(f"{name} s={s}: {cls} q={f} lies outside its bracket")
        for _ in range(args.warmup):
            sketch()
        ms = timed(sketch, args.reps)
        med = statistics.median(ms)
        e = {"kind": "whole batch", "input": name, "why": qb.INPUTS[name][2], "n_records": n, "sub_bits": s,
             "table_bytes": isim.sketch_words(s) * 8, "bins_hit": int((got != 0).sum()),
             "p99_exact_ns": exact["all"]["q"][0.99], "p99_bracket_ns": list(brackets["all"]["q"][0.99]),
             "sketch": spread(ms), "bytes": n * 16, "sketch_gbs": n * 16 / (med * 1e-3) / 1e9,
             "exact_select": spread(sel), "copy_d2h_pinned": spread(copy_ms),
             "select_over_sketch": statistics.median(sel) / med,
             "copy_over_sketch": statistics.median(copy_ms) / med,
             "sketch_faster_than_select": bool(max(ms) < min(sel)),
             "sketch_faster_than_copy": bool(max(ms) < min(copy_ms))}
        print(json.dumps(e), flush=True)
        entries.append(e)
    return entries


def measure_windows(name, args, torch, dev):
    import numpy as np

    import isim
    import timeline_bench as tb
    import timeline_quantiles_bench as tqb
    U = np.uint64
    stream = torch.cuda.current_stream(dev)
    timed = timer(torch, stream)
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

    p_rec = torch.empty((n, 2), dtype=torch.int64, pin_memory=True)
    p_arr = torch.empty(n, dtype=torch.int64, pin_memory=True)

    def copy():
        p_rec.copy_(recs, non_blocking=True)
        p_arr.copy_(arr, non_blocking=True)

    copy()
    torch.cuda.synchronize()
    copy_ms = timed(copy, 5)
    h_arr = p_arr.numpy().view(U)
    h_rec = p_rec.numpy().view(isim.REC_DTYPE).reshape(n)
    lat = h_rec["latency_ns"]
    span = int(h_arr.max()) + int(lat.max())
    code = (h_rec["status_err"] >> np.uint32(31)).astype(np.int64)
    c = h_arr + lat
    c[c < h_arr] = U((1 << 64) - 1)

    entries = []
    for wname, window in WINDOWS.items():
        n_windows = max(1, min(isim.native.TL_MAX_WINDOWS, span // window + 1))
        rc = (np.minimum(c // U(window), U(n_windows)) + U(1)).astype(np.int64)  # t0 = 0
        # baseline 1: the exact per-window select, unchanged
        words = isim.timeline_quantiles_out_words(n_windows, len(tqb.Q))
        qout = torch.empty(words, dtype=torch.int64, device=dev)
        wsb = isim.timeline_quantiles_workspace_bytes(n, n_windows, len(tqb.Q))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

        def tlq():
            isim.timeline_quantiles_device(arr.data_ptr(), recs.data_ptr(), n, window, n_windows, 0, tqb.Q,
                                           d_out=qout.data_ptr(), d_workspace=ws.data_ptr(), workspace_bytes=wsb,
                                           stream=stream.cuda_stream)

        for _ in range(args.warmup):
            tlq()
        exact_ms = timed(tlq, args.reps)
        del qout, ws
        for s in SUB_BITS:
            out = torch.zeros(isim.timeline_sketch_out_words(n_windows, s), dtype=torch.int64, device=dev)

            def sketch():
                isim.timeline_sketch_device(arr.data_ptr(), recs.data_ptr(), n, window, n_windows, 0, s,
                                            d_out=out.data_ptr(), stream=stream.cuda_stream)

            sketch()
            got = out.cpu().numpy().view(U)
            bins = isim.sketch_bins(s)
            if not same_table(np, got, (rc * 2 + code) * bins + bucket_np(s, lat)):
                raise SystemExit(f"{name} {wname} s={s}: the device table differs from the host's")
            per_row = got.reshape(n_windows + 2, 2 * bins).sum(axis=1)
            for _ in range(args.warmup):
                sketch()
            ms = timed(sketch, args.reps)
            med = statistics.median(ms)
            e = {"kind": "per window", "input": name, "why": tb.INPUTS[name][1], "n_records": n, "window": wname,
                 "window_ns": window, "n_windows": n_windows, "sub_bits": s,
                 "lds_rows": min(n_windows + 2, 7424 // bins), "rows_hit": int((per_row > 0).sum()),
                 "longest_row": int(per_row.max()), "after_row": int(per_row[-1]), "table_bytes": got.size * 8,
                 "sketch": spread(ms), "bytes": n * 24, "sketch_gbs": n * 24 / (med * 1e-3) / 1e9,
                 "exact_timeline_quantiles": spread(exact_ms), "copy_d2h_pinned": spread(copy_ms),
                 "exact_over_sketch": statistics.median(exact_ms) / med,
                 "copy_over_sketch": statistics.median(copy_ms) / med,
                 "sketch_faster_than_exact": bool(max(ms) < min(exact_ms)),
                 "sketch_faster_than_copy": bool(max(ms) < min(copy_ms))}
            print(json.dumps(e), flush=True)
            entries.append(e)
            del out, got
    return entries


def worker(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sketch_bench needs a GPU: it measures, it does not fall back")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    entries = []
    for name in names(args.batch_inputs):
        entries += measure_batch(name, args, torch, dev)
        torch.cuda.empty_cache()
    for name in names(args.window_inputs):
        entries += measure_windows(name, args, torch, dev)
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(dev), "warmup": args.warmup, "sub_bits": list(SUB_BITS),
           "timing": "HIP events around one call; every baseline in the same process on the same batch",
           "kernels": RESOURCES, "kernels_note": RESOURCES_NOTE, "entries": entries}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


def main():
    args = parse()
    import quantile_bench as qb
    import timeline_bench as tb
    for name in names(args.batch_inputs):
        if name not in qb.INPUTS:
            raise SystemExit(f"unknown whole-batch input {name!r}: one of {', '.join(qb.INPUTS)}")
    for name in names(args.window_inputs):
        if name not in tb.INPUTS:
            raise SystemExit(f"unknown per-window input {name!r}: one of {', '.join(tb.INPUTS)}")
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
