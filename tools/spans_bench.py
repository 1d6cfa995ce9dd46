"""Timing of the tail select and the span walks (isim_select_traces_device,
isim_trace_spans_device) on a served config-3p batch of 2^22
traces: the exact p99.9 threshold from isim_latency_quantiles_device, the
select of the traces at or above it, and the spans of the selected ids.  Next
to those, in the same process, isim_serve_device of as many traces as were
selected: the ordinary walk of the same work is the yardstick (no ratio is
fixed in advance).

Each device call is timed with HIP events (--warmup calls, then --reps: median,
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
    ap.add_argument("--log2n", type=int, default=22, help="traces of the served batch")
    ap.add_argument("--q-ppm", type=int, default=999000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spans_bench.json"))
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

    recs, stats = i64(2 * n), i64(h.stats_words)
    h.serve_device(0, n, recs.data_ptr(), stats.data_ptr(), stream)
    qout = i64(isim.quantiles_out_words(1))
    qws = torch.empty(isim.quantiles_workspace_bytes(1), dtype=torch.uint8, device=dev)
    isim.latency_quantiles_device(recs.data_ptr(), n, (a.q_ppm / 1e6,), d_out=qout.data_ptr(),
                                  d_workspace=qws.data_ptr(), stream=stream)
    thr = int(qout.cpu().numpy().view(np.uint64).reshape(3, 2)[native.Q_ALL, 1])
    ids, sinfo = i64(n), i64(2)
    sws = torch.empty(isim.select_workspace_bytes(n), dtype=torch.uint8, device=dev)

    def select():
        isim.select_traces_device(recs.data_ptr(), n, 0, thr, native.Q_ALL, max_ids=n, d_ids=ids.data_ptr(),
                                  d_info=sinfo.data_ptr(), d_workspace=sws.data_ptr(), stream=stream)

    t_select = timed(select)
    m = int(sinfo.cpu().numpy().view(np.uint64)[1])
    off, info = i64(m + 1), i64(native.SPAN_INFO_WORDS)
    wsb = ts.workspace_bytes(m)
    ws = torch.empty(max(1, wsb), dtype=torch.uint8, device=dev)
    ts.spans_device(ids.data_ptr(), m, d_off=off.data_ptr(), d_spans=0, cap_spans=0, d_info=info.data_ptr(),
                    d_workspace=ws.data_ptr(), workspace_bytes=wsb, stream=stream)
    total = int(info.cpu().numpy().view(np.uint64)[native.SPAN_TOTAL])
    spans = torch.empty(max(1, total) * 48, dtype=torch.uint8, device=dev)

    def walk():
        ts.spans_device(ids.data_ptr(), m, d_off=off.data_ptr(), d_spans=spans.data_ptr(), cap_spans=total,
                        d_info=info.data_ptr(), d_workspace=ws.data_ptr(), workspace_bytes=wsb, stream=stream)

    t_spans = timed(walk)
    assert int(info.cpu().numpy().view(np.uint64)[native.SPAN_WRITTEN]) == m

    def serve_m():
        h.serve_device(0, m, recs.data_ptr(), stats.data_ptr(), stream)

    def serve_n():
        h.serve_device(0, n, recs.data_ptr(), stats.data_ptr(), stream)

    out = {"device": torch.cuda.get_device_name(0), "graph": "config3p_topology()", "n_traces": n, "q_ppm": a.q_ppm,
           "threshold_ns": thr, "selected": m, "spans": total, "span_bytes": total * 48,
           "select": t_select, "spans_of_selected": t_spans,
           "serve_device_same_count": timed(serve_m), "serve_device_batch": timed(serve_n)}
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
        print(f"spans_bench: the measuring process passed its limit of {a.timeout} s", file=sys.stderr)
        rc = 124
    sys.exit(rc)


if __name__ == "__main__":
    main()
