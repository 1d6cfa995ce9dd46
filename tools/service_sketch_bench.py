"""Timing of the per-service latency sketch (isim_service_sketch_device, DESIGN.md
§30) on a whole tapped DES batch (threshold 0, every trace): --graph c5p
(bench.py's config 5p, 10,000 services) or --graph tree13 (a 13-service tree
under overload, one long segment per service), at each of --sub-bits.  In one
process, on the same spans: the device call; isim_service_quantiles_device (the
exact select the sketch stands next to); and the pinned device-to-host copy of
the spans (through one pinned buffer of --pinned-mib) followed by the host's
fold (isim_service_sketch_host, once), which is what a host-side route pays.
Each device table is compared with the host's, word for word, before its time
is accepted, and after the timed calls it must be that table times the number
of calls.  The share of segments and spans in each tier is reported.  No ratio
is fixed in advance.

The device calls are timed with HIP events (--warmup calls, then --reps: median,
min and max).  The parent process never opens the GPU: it starts the measuring
process under a time limit (--timeout) and reports its exit status.  The result
is merged into --out under the graph's name.
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
    ap.add_argument("--mean-ns", type=int, default=None, help="mean gap (default: bench.py's 6 ms for c5p, 700 us for tree13)")
    ap.add_argument("--sub-bits", default="3,7")
    ap.add_argument("--q", default="0.5,0.9,0.99,0.999", help="the quantiles of the exact select timed next to it")
    ap.add_argument("--pinned-mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=900, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "service_sketch_bench.json"))
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
    from isim.service_sketch import service_sketch_device, service_sketch_table_words, service_sketch_workspace_bytes
    from service_quantiles_bench import tree13

    dev = torch.device("cuda", 0)
    torch.cuda.init()
    stream = torch.cuda.current_stream(dev).cuda_stream
    q = tuple(float(x) for x in a.q.split(","))
    short = native.SVS_SHORT
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

    def i64(words):
        return torch.zeros(max(1, words), dtype=torch.int64, device=dev)

    ws = torch.empty(d.workspace_bytes(n) + 8, dtype=torch.uint8, device=dev)
    recs, stats, table = i64(2 * n), i64(len(h.new_stats())), i64(d.table_words)
    ids, off, info = i64(n), i64(n + 1), i64(native.DES_SPAN_INFO_WORDS)
    wide = [False]

    def des(t):
        d.serve_spans_device(1 << 31, n, recs.data_ptr(), stats.data_ptr(), table.data_ptr(), ws.data_ptr(),
                             ws.numel(), t, stream, wide=wide[0])

    # a tap without room counts the batch's spans first
    count_tap = make_tap(0, 0, native.Q_ALL, n, 0, ids.data_ptr(), off.data_ptr(), 0, info.data_ptr())
    des(count_tap)
    torch.cuda.synchronize()
    if int(stats.cpu().numpy().view(np.uint64)[native.ST_DES_RETRY]):
        wide[0] = True
        stats.zero_()
        des(count_tap)
        torch.cuda.synchronize()
    cap = int(info.cpu().numpy().view(np.uint64)[native.SPAN_TOTAL])
    spans = torch.empty(cap * 64, dtype=torch.uint8, device=dev)
    des(make_tap(0, 0, native.Q_ALL, n, cap, ids.data_ptr(), off.data_ptr(), spans.data_ptr(), info.data_ptr()))
    torch.cuda.synchronize()
    word = info.cpu().numpy().view(np.uint64)
    total = int(word[native.SPAN_TOTAL])
    assert int(word[native.SPAN_WRITTEN]) == n == int(word[native.DES_SPAN_MATCHES]) and total <= cap

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

    # the two baselines: the exact select, and the pinned copy with the host's fold
    qwords = service_quantiles_table_words(h, len(q))
    qws_bytes = service_quantiles_workspace_bytes(h, cap, len(q))
    qout, qws = i64(qwords), torch.empty(qws_bytes + 8, dtype=torch.uint8, device=dev)
    t_sel = timed(lambda: service_quantiles_device(h, q, off.data_ptr(), spans.data_ptr(), cap, info.data_ptr(),
                                                   qout.data_ptr(), qws.data_ptr(), qws_bytes, stream))
    del qws
    chunk = min(total * 64, a.pinned_mib << 20)
    pinned = torch.empty(chunk, dtype=torch.uint8).pin_memory()

    def copy():
        for lo in range(0, total * 64, chunk):
            hi = min(total * 64, lo + chunk)
            pinned[:hi - lo].copy_(spans[lo:hi], non_blocking=True)

    t_copy = timed(copy, warmup=1, reps=5)
    h_spans = spans.cpu().numpy().view(isim.DES_SPAN_DTYPE)[:total]
    ok = (h_spans["service"] < h.info.n_services) & (h_spans["arrival_ns"] <= h_spans["start_ns"]) \
        & (h_spans["start_ns"] <= h_spans["finish_ns"])
    seg = np.bincount(h_spans["service"][ok], minlength=int(h.info.n_services))
    long_, short_ = seg > short, (seg > 0) & (seg <= short)
    tiers = {"short_bound": short, "chunk": native.SVQ_CHUNK,
             "segments": {"long": int(long_.sum()), "short": int(short_.sum()), "empty": int((seg == 0).sum()),
                          "median": int(np.median(seg)), "max": int(seg.max())},
             "spans": {"long": int(seg[long_].sum()), "short": int(seg[short_].sum())},
             "share_of_segments": {"long": float(long_.sum() / max(1, (seg > 0).sum())),
                                   "short": float(short_.sum() / max(1, (seg > 0).sum()))},
             "share_of_spans": {"long": float(seg[long_].sum() / max(1, seg.sum())),
                                "short": float(seg[short_].sum() / max(1, seg.sum()))},
             "long_chunks": int(((seg[long_] - 1) // native.SVQ_CHUNK + 1).sum())}

    kws_bytes = service_sketch_workspace_bytes(h, cap)
    kws = torch.empty(kws_bytes + 8, dtype=torch.uint8, device=dev)
    per_s = {}
    for s in [int(x) for x in a.sub_bits.split(",")]:
        words = service_sketch_table_words(h, s)
        out = i64(words)

        def sketch():
            service_sketch_device(h, s, off.data_ptr(), spans.data_ptr(), cap, info.data_ptr(), out.data_ptr(),
                                  kws.data_ptr(), kws_bytes, stream)

        sketch()
        torch.cuda.synchronize()
        dev_table = out.cpu().numpy().view(np.uint64).copy()
        t0 = time.perf_counter()
        host_table = isim.service_sketch_host(h, h_spans, s)
        host_s = time.perf_counter() - t0
        bad = np.flatnonzero(host_table != dev_table)
        assert bad.size == 0, (s, bad[:4], host_table[bad[:4]], dev_table[bad[:4]])
        t_sk = timed(sketch)
        torch.cuda.synchronize()
        calls = 1 + a.warmup + a.reps
        assert np.array_equal(out.cpu().numpy().view(np.uint64), dev_table * np.uint64(calls))   # every call added the same
        per_s[str(s)] = {"table_words": int(words),
                         "service_sketch_device": dict(t_sk, ns_per_span=1e6 * t_sk["median_ms"] / max(1, total)),
                         "host_fold_s": host_s, "compared_with_host": True,
                         "sketch_over_select": t_sk["median_ms"] / t_sel["median_ms"],
                         "sketch_over_copy": t_sk["median_ms"] / t_copy["median_ms"],
                         "sketch_over_copy_and_host_fold": t_sk["median_ms"] / (t_copy["median_ms"] + 1e3 * host_s)}
        del out

    res = {"device": torch.cuda.get_device_name(0), "n_traces": n, "mean_ns": mean, "n_services": int(h.info.n_services),
           "spans": total, "span_bytes": total * 64, "tiers": tiers, "workspace_bytes": int(kws_bytes),
           "library": os.path.basename(native.LIB_PATH), "sub_bits": per_s,
           "service_quantiles_device": dict(t_sel, q=list(q)),
           "pinned_copy": dict(t_copy, pinned_buffer_bytes=int(chunk), bytes_per_s=total * 64 / (1e-3 * t_copy["median_ms"]))}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc[a.graph] = res
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
        print(f"service_sketch_bench: the measuring process passed its limit of {a.timeout} s", file=sys.stderr)
        rc = 124
    sys.exit(rc)


if __name__ == "__main__":
    main()
