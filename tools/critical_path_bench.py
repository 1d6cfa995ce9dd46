"""Timing of isim_critical_path_device on the batch of
tools/spans_bench.py: a served config-3p batch of 2^22 traces, the traces at or
above its exact p99.9, their spans.  Next to it, in the same process, the two
yardsticks: isim_trace_spans_device of the same list (the call that produces the
spans the fold reads), and the way without the device fold, a copy of the spans
to pinned host memory plus isim_critical_path_host.  No ratio is fixed in
advance.

The device calls are timed with HIP events (--warmup calls, then --reps: median,
min and max), the host fold with a wall clock.  The fold works in place, so every
timed fold follows an untimed span call that writes the spans afresh.  The parent
process never opens the GPU: it starts the measuring process under a time limit
(--timeout) and reports its exit status.
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


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2n", type=int, default=22, help="traces of the served batch")
    ap.add_argument("--q-ppm", type=int, default=999000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3, help="timed runs of the copy and of the host fold")
    ap.add_argument("--timeout", type=int, default=420, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "critical_path_bench.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def worker(a):
    import numpy as np
    import torch

    import isim
    from isim import native
    from isim.generators import config3p_topology
    from isim.yamljson import obj_to_json

    dev = torch.device("cuda", 0)
    torch.cuda.init()
    stream = torch.cuda.current_stream(dev).cuda_stream
    h = isim.Handler(isim.ServiceGraph.from_json(obj_to_json(config3p_topology())), None, isim.SimParams())
    ts = isim.TraceSpans(h)
    n = 1 << a.log2n

    def i64(words):
        return torch.zeros(max(1, words), dtype=torch.int64, device=dev)

    def timed(fn, before=None):
        ms = []
        for r in range(a.warmup + a.reps):
            if before:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return spread(ms)

    recs, stats = i64(2 * n), i64(h.stats_words)
    h.serve_device(0, n, recs.data_ptr(), stats.data_ptr(), stream)
    qout = i64(isim.quantiles_out_words(1))
    qws = torch.empty(isim.quantiles_workspace_bytes(1), dtype=torch.uint8, device=dev)
    isim.latency_quantiles_device(recs.data_ptr(), n, (a.q_ppm / 1e6,), d_out=qout.data_ptr(),
                                  d_workspace=qws.data_ptr(), stream=stream)
    thr = int(qout.cpu().numpy().view(np.uint64).reshape(3, 2)[native.Q_ALL, 1])
    ids, sinfo = i64(n), i64(2)
    sws = torch.empty(isim.select_workspace_bytes(n), dtype=torch.uint8, device=dev)
    isim.select_traces_device(recs.data_ptr(), n, 0, thr, native.Q_ALL, max_ids=n, d_ids=ids.data_ptr(),
                              d_info=sinfo.data_ptr(), d_workspace=sws.data_ptr(), stream=stream)
    m = int(sinfo.cpu().numpy().view(np.uint64)[1])
    off, info = i64(m + 1), i64(native.SPAN_INFO_WORDS)
    wsb = ts.workspace_bytes(m)
    ws = torch.empty(max(1, wsb), dtype=torch.uint8, device=dev)
    ts.spans_device(ids.data_ptr(), m, d_off=off.data_ptr(), d_spans=0, cap_spans=0, d_info=info.data_ptr(),
                    d_workspace=ws.data_ptr(), workspace_bytes=wsb, stream=stream)
    total = int(info.cpu().numpy().view(np.uint64)[native.SPAN_TOTAL])
    spans = torch.empty(max(1, total) * 48, dtype=torch.uint8, device=dev)
    cwb = ts.critical_path_workspace_bytes(total)
    cws = torch.empty(cwb, dtype=torch.uint8, device=dev)
    table = i64(ts.table_words())

    def walk():
        ts.spans_device(ids.data_ptr(), m, d_off=off.data_ptr(), d_spans=spans.data_ptr(), cap_spans=total,
                        d_info=info.data_ptr(), d_workspace=ws.data_ptr(), workspace_bytes=wsb, stream=stream)

    def fold():
        ts.critical_path_device(d_off=off.data_ptr(), d_spans=spans.data_ptr(), cap_spans=total, d_info=info.data_ptr(),
                                n_ids=m, d_table=table.data_ptr(), d_workspace=cws.data_ptr(), workspace_bytes=cwb,
                                stream=stream)

    t_spans = timed(walk)
    assert int(info.cpu().numpy().view(np.uint64)[native.SPAN_WRITTEN]) == m
    t_fold = timed(fold, before=walk)
    d_table = table.cpu().numpy().view(np.uint64).reshape(-1, native.CP_ROW_WORDS)
    calls = a.warmup + a.reps

    # the way without the device fold: the spans to pinned host memory, the fold on the CPU
    h_spans = torch.empty(max(1, total) * 48, dtype=torch.uint8).pin_memory()
    h_off = off.cpu().numpy().view(np.uint64).copy()
    walk()
    copy_ms, host_ms = [], []
    for _ in range(a.host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h_spans.copy_(spans[:max(1, total) * 48], non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        h_table = ts.fold_host(h_off, h_spans.numpy().view(isim.SPAN_DTYPE)[:total], m)
        t2 = time.perf_counter()
        copy_ms.append((t1 - t0) * 1e3)
        host_ms.append((t2 - t1) * 1e3)
    h_table = h_table.reshape(-1, native.CP_ROW_WORDS)
    # every device call added the same table; the host's is one call's
    assert np.array_equal(d_table, h_table * np.uint64(calls)), "device and host tables differ"

    rows = isim.CriticalPath(h, h_table, ts.names).rows()
    out = {"device": torch.cuda.get_device_name(0), "graph": "config3p_topology()", "n_traces": n, "q_ppm": a.q_ppm,
           "threshold_ns": thr, "selected": m, "spans": total, "span_bytes": total * 48,
           "critical_spans": int(h_table[-1, native.CP_H_CRITICAL]),
           "spans_of_selected": t_spans, "critical_path_device": t_fold,
           "copy_to_pinned_host": spread(copy_ms), "critical_path_host": spread(host_ms),
           "top_services": [{k: r[k] for k in ("service", "share", "critical", "invocations")} for r in rows[:5]]}
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
        print(f"critical_path_bench: the measuring process passed its limit of {a.timeout} s", file=sys.stderr)
        rc = 124
    sys.exit(rc)


if __name__ == "__main__":
    main()
