"""Timing of the service timeline fold (isim_service_timeline_device, DESIGN.md
§23): a config-5p DES step of 2^19 traces under a two-step load profile, the
whole batch tapped (threshold 0, every trace).  Three timings in one process:
the tap of the whole batch against the NULL tap, the device fold with windows
of 1 ms and of 1 us, and the pinned device-to-host copy of the same spans (64 B
each, through one pinned buffer of --pinned-mib), which any host-side
alternative pays before it starts.  No ratio is fixed in advance.

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
    ap.add_argument("--step-mean-ns", type=int, default=4_000_000, help="the gap during the profile's second step")
    ap.add_argument("--n-windows", type=int, default=1024, help="c5p has 10,000 services: at most 2^24 cells")
    ap.add_argument("--pinned-mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=500, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "service_timeline_bench.json"))
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
    from isim.service_timeline import (service_timeline_device, service_timeline_table_words,
                                       service_timeline_workspace_bytes)

    dev = torch.device("cuda", 0)
    torch.cuda.init()
    stream = torch.cuda.current_stream(dev).cuda_stream
    j, _ = bench.build_graph("c5p")
    h = isim.Handler(isim.ServiceGraph.from_json(j), None, isim.SimParams())
    n = 1 << a.log2n
    # a third of the batch at the base gap, a sixth at the step's, the rest at the base gap again
    t_step = (n // 3) * a.mean_ns
    prof = isim.LoadProfile.steps([(t_step, a.mean_ns), ((n // 6) * a.step_mean_ns, a.step_mean_ns)], a.mean_ns)
    d = isim.DesHandler(h, profile=prof)
    assert d.info.items == 1

    def i64(words):
        return torch.zeros(max(1, words), dtype=torch.int64, device=dev)

    ws = torch.empty(d.workspace_bytes(n) + 8, dtype=torch.uint8, device=dev)
    recs, stats, table = i64(2 * n), i64(len(h.new_stats())), i64(d.table_words)
    ids, off, info = i64(n), i64(n + 1), i64(native.DES_SPAN_INFO_WORDS)

    def call(t):
        d.serve_spans_device(1 << 31, n, recs.data_ptr(), stats.data_ptr(), table.data_ptr(), ws.data_ptr(),
                             ws.numel(), t, stream)

    # hops_upper spans per trace would be 312 GiB here: a tap without room counts the batch's spans first
    call(make_tap(0, 0, native.Q_ALL, n, 0, ids.data_ptr(), off.data_ptr(), 0, info.data_ptr()))
    torch.cuda.synchronize()
    cap = int(info.cpu().numpy().view(np.uint64)[native.SPAN_TOTAL])
    spans = torch.empty(cap * 64, dtype=torch.uint8, device=dev)
    tap = make_tap(0, 0, native.Q_ALL, n, cap, ids.data_ptr(), off.data_ptr(), spans.data_ptr(), info.data_ptr())

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
    total = int(word[native.SPAN_TOTAL])
    assert int(word[native.SPAN_WRITTEN]) == n == int(word[native.DES_SPAN_MATCHES]) and total <= cap
    assert not int(stats.cpu().numpy().view(np.uint64)[native.ST_DES_RETRY])

    folds = {}
    for name, window in (("window_1ms", 1_000_000), ("window_1us", 1_000)):
        words = service_timeline_table_words(h, window, a.n_windows, t_step)
        tws_bytes = service_timeline_workspace_bytes(h, window, a.n_windows, t_step)
        out, tws = i64(words), torch.empty(tws_bytes, dtype=torch.uint8, device=dev)

        def fold():
            service_timeline_device(h, window, a.n_windows, t_step, off.data_ptr(), spans.data_ptr(), cap,
                                    info.data_ptr(), out.data_ptr(), tws.data_ptr(), tws_bytes, stream)

        t = timed(fold)
        out.zero_()
        fold()
        torch.cuda.synchronize()
        tab = out.cpu().numpy().view(np.uint64)
        rows = tab[:-native.SVT_ROW_WORDS].reshape(h.info.n_services, a.n_windows + 2, native.SVT_ROW_WORDS)
        assert int(tab[-native.SVT_ROW_WORDS + native.SVT_H_FOLDED]) == total
        assert int(rows[:, :, native.SVT_ARRIVED].sum()) == total
        assert int(rows[:, :, native.SVT_QUEUED_NS].sum(dtype=np.uint64)) == int(rows[:, :, native.SVT_SUM_WAIT].sum(dtype=np.uint64))
        folds[name] = dict(t, window_ns=window, table_words=int(words), workspace_bytes=int(tws_bytes),
                           ns_per_span=1e6 * t["median_ms"] / total,
                           span_bytes_per_s=total * 64 / (1e-3 * t["median_ms"]))

    chunk = min(total * 64, a.pinned_mib << 20)
    pinned = torch.empty(chunk, dtype=torch.uint8).pin_memory()

    def copy():
        for lo in range(0, total * 64, chunk):
            hi = min(total * 64, lo + chunk)
            pinned[:hi - lo].copy_(spans[lo:hi], non_blocking=True)

    t_copy = timed(copy)
    out = {"device": torch.cuda.get_device_name(0), "graph": "bench.build_graph('c5p')", "n_traces": n,
           "profile": {"base_mean_ns": a.mean_ns, "step_mean_ns": a.step_mean_ns, "step_begins_ns": t_step},
           "spans": total, "span_bytes": total * 64, "n_windows": a.n_windows, "t0_ns": t_step,
           "null_tap": t_null, "whole_batch_tap": t_tap, "tap_over_null": t_tap["median_ms"] / t_null["median_ms"],
           "fold": folds, "pinned_copy": dict(t_copy, pinned_buffer_bytes=int(chunk),
                                              bytes_per_s=total * 64 / (1e-3 * t_copy["median_ms"])),
           "fold_1ms_over_copy": folds["window_1ms"]["median_ms"] / t_copy["median_ms"],
           "fold_1us_over_copy": folds["window_1us"]["median_ms"] / t_copy["median_ms"]}
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
        print(f"service_timeline_bench: the measuring process passed its limit of {a.timeout} s", file=sys.stderr)
        rc = 124
    sys.exit(rc)


if __name__ == "__main__":
    main()
