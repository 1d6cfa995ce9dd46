"""Timing of the per-service percentiles over time (isim_service_window_quantiles_device,
DESIGN.md §29) on a whole tapped DES batch (threshold 0, every trace) of --graph
c5p (bench.py's config 5p, 10,000 services) or tree13 (a 13-service tree under
overload).  In one process, per entry of --windows (windows that together cover
the batch's finishes): the device call; and once isim_service_quantiles_device
over the same spans (§28, the floor for one window), the pinned device-to-host
copy of the spans and, for the first entry of --windows, the host's table
(isim_service_window_quantiles_host), which is what a host-side route pays.  Every
device table is compared with the host's, word for word, before its time is
accepted (--no-host skips both).  The share of cells in each tier is read from
the table's counts.  No ratio is fixed in advance.

The device calls are timed with HIP events (--warmup calls, then --reps: median,
min and max).  The parent process never opens the GPU: it starts the measuring
process under a time limit (--timeout) and reports its exit status.  The result
is merged into --out under --key (default: the graph's name).  --calls-only N
taps the batch, makes N device calls at the first entry of --windows and leaves:
the process a kernel trace is taken of.
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


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graph", choices=["c5p", "tree13"], default="c5p")
    ap.add_argument("--log2n", type=int, default=19, help="traces of the DES step")
    ap.add_argument("--mean-ns", type=int, default=None, help="mean gap (default: 6 ms for c5p, 700 us for tree13)")
    ap.add_argument("--q", default="0.5,0.9,0.99,0.999")
    ap.add_argument("--windows", default="1,64,1024", help="numbers of windows; one above ISIM_SWQ_MAX_CELLS for the "
                    "graph is reported as refused")
    ap.add_argument("--pinned-mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the host tables (and with them the comparison)")
    ap.add_argument("--key", default=None)
    ap.add_argument("--wave", type=int, default=None, help="ISIM_SWQ_WAVE of a library variant chosen with ISIM_LIB")
    ap.add_argument("--calls-only", type=int, default=0, metavar="N")
    ap.add_argument("--timeout", type=int, default=900, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "service_window_quantiles_bench.json"))
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
    from isim.service_quantiles import (service_quantiles_device, service_quantiles_table_words,
                                        service_quantiles_workspace_bytes)
    from isim.service_window_quantiles import (service_window_quantiles_device, service_window_quantiles_host,
                                               service_window_quantiles_table_words,
                                               service_window_quantiles_workspace_bytes)
    from service_quantiles_bench import tree13

    dev = torch.device("cuda", 0)
    torch.cuda.init()
    stream = torch.cuda.current_stream(dev).cuda_stream
    q = tuple(float(x) for x in a.q.split(","))
    if a.graph == "c5p":
        j, _ = bench.build_graph("c5p")
        h = isim.Handler(isim.ServiceGraph.from_json(j), None, isim.SimParams())
        mean = a.mean_ns or 6_000_000
    else:
        h = isim.Handler(isim.ServiceGraph.from_json(tree13()), None, isim.SimParams(flags=native.FLAG_DYNAMIC))
        mean = a.mean_ns or 700_000
    d = isim.DesHandler(h, mean)
    assert d.info.items == 1
    n = 1 << a.log2n
    ns = int(h.info.n_services)

    def i64(words):
        return torch.zeros(max(1, words), dtype=torch.int64, device=dev)

    ws = torch.empty(d.workspace_bytes(n) + 8, dtype=torch.uint8, device=dev)
    recs, stats, table = i64(2 * n), i64(len(h.new_stats())), i64(d.table_words)
    ids, off, info = i64(n), i64(n + 1), i64(native.DES_SPAN_INFO_WORDS)
    wide = [False]

    def call(t):
        d.serve_spans_device(1 << 31, n, recs.data_ptr(), stats.data_ptr(), table.data_ptr(), ws.data_ptr(),
                             ws.numel(), t, stream, wide=wide[0])

    # a tap without room counts the batch's spans first
    count_tap = make_tap(0, 0, native.Q_ALL, n, 0, ids.data_ptr(), off.data_ptr(), 0, info.data_ptr())
    call(count_tap)
    torch.cuda.synchronize()
    if int(stats.cpu().numpy().view(np.uint64)[native.ST_DES_RETRY]):
        wide[0] = True
        stats.zero_()
        call(count_tap)
        torch.cuda.synchronize()
    cap = int(info.cpu().numpy().view(np.uint64)[native.SPAN_TOTAL])
    spans = torch.empty(cap * 64, dtype=torch.uint8, device=dev)
    call(make_tap(0, 0, native.Q_ALL, n, cap, ids.data_ptr(), off.data_ptr(), spans.data_ptr(), info.data_ptr()))
    torch.cuda.synchronize()
    word = info.cpu().numpy().view(np.uint64)
    total = int(word[native.SPAN_TOTAL])
    assert int(word[native.SPAN_WRITTEN]) == n == int(word[native.DES_SPAN_MATCHES]) and total <= cap
    h_spans = spans.cpu().numpy().view(isim.DES_SPAN_DTYPE)[:total]
    last = int(h_spans["finish_ns"].max())

    def timed(fn, warmup=a.warmup, reps=a.reps):
        for _ in range(warmup):
            fn()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return spread(ms)

    wave = a.wave or native.SWQ_WAVE
    res = {"device": torch.cuda.get_device_name(0), "n_traces": n, "mean_ns": mean, "q": list(q), "n_services": ns,
           "spans": total, "span_bytes": total * 64, "library": os.path.basename(native.LIB_PATH),
           "wave": wave, "windows": {}}
    for k, nw in enumerate(int(x) for x in a.windows.split(",")):
        window = last // nw + 1       # the windows cover every finish
        if ns * (nw + 2) > native.SWQ_MAX_CELLS:
            res["windows"][str(nw)] = {"refused": f"{ns * (nw + 2)} cells are above ISIM_SWQ_MAX_CELLS"}
            continue
        words = service_window_quantiles_table_words(h, len(q), window, nw, 0)
        ws_bytes = service_window_quantiles_workspace_bytes(h, cap, len(q), window, nw, 0)
        out = torch.full((words,), -1, dtype=torch.int64, device=dev)
        qws = torch.empty(ws_bytes + 8, dtype=torch.uint8, device=dev)

        def select():
            service_window_quantiles_device(h, q, window, nw, 0, off.data_ptr(), spans.data_ptr(), cap,
                                            info.data_ptr(), out.data_ptr(), qws.data_ptr(), ws_bytes, stream)

        select()
        torch.cuda.synchronize()
        dev_table = out.cpu().numpy().view(np.uint64).copy()
        if a.calls_only:
            for _ in range(a.calls_only):
                select()
            torch.cuda.synchronize()
            return
        host = None
        if not a.no_host:
            t0 = time.perf_counter()
            host_table = service_window_quantiles_host(h, h_spans, q, window, nw, 0)
            host = time.perf_counter() - t0
            bad = np.flatnonzero(host_table != dev_table)
            assert bad.size == 0, (nw, bad[:4], host_table[bad[:4]], dev_table[bad[:4]])
        t_sel = timed(select)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), dev_table)     # every timed call wrote the same table
        seg = dev_table[:-2].reshape(-1, 3, 3, 1 + len(q))[:, 0, 0, 0]
        tiers = {"empty": int((seg == 0).sum()), "wave": int(((seg > 0) & (seg <= wave)).sum()),
                 "lds": int(((seg > wave) & (seg <= native.SVQ_STAGE)).sum()),
                 "long": int((seg > native.SVQ_STAGE).sum())}
        in_tier = {"wave": int(seg[seg <= wave].sum()),
                   "lds": int(seg[(seg > wave) & (seg <= native.SVQ_STAGE)].sum()),
                   "long": int(seg[seg > native.SVQ_STAGE].sum())}
        res["windows"][str(nw)] = dict(t_sel, window_ns=window, cells=int(seg.size), cells_by_tier=tiers,
                                       spans_by_tier=in_tier, table_words=int(words), workspace_bytes=int(ws_bytes),
                                       ns_per_span=1e6 * t_sel["median_ms"] / max(1, total), host_table_s=host,
                                       compared_with_host=host is not None)
        del out, qws

    words = service_quantiles_table_words(h, len(q))
    sws_bytes = service_quantiles_workspace_bytes(h, cap, len(q))
    sout, sws = i64(words), torch.empty(sws_bytes + 8, dtype=torch.uint8, device=dev)
    res["service_quantiles_device"] = timed(lambda: service_quantiles_device(
        h, q, off.data_ptr(), spans.data_ptr(), cap, info.data_ptr(), sout.data_ptr(), sws.data_ptr(), sws_bytes, stream))
    chunk = min(total * 64, a.pinned_mib << 20)
    pinned = torch.empty(chunk, dtype=torch.uint8).pin_memory()

    def copy():
        for lo in range(0, total * 64, chunk):
            hi = min(total * 64, lo + chunk)
            pinned[:hi - lo].copy_(spans[lo:hi], non_blocking=True)

    t_copy = timed(copy, warmup=1, reps=5)
    res["pinned_copy"] = dict(t_copy, bytes_per_s=total * 64 / (1e-3 * t_copy["median_ms"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc[a.key or a.graph] = res
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def main():
    a = parse()
    if a.worker:
        return worker(a)
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"] + sys.argv[1:],
                            timeout=a.timeout).returncode
    except subprocess.TimeoutExpired:
        print(f"service_window_quantiles_bench: the measuring process passed its limit of {a.timeout} s", file=sys.stderr)
        rc = 124
    sys.exit(rc)


if __name__ == "__main__":
    main()
