"""Timing of the per-service percentiles (isim_service_quantiles_device, DESIGN.md
§28) on a whole tapped DES batch (threshold 0, every trace): --graph c5p
(bench.py's config 5p, 10,000 services) or --graph tree13 (a 13-service tree
under overload, one long segment per service).  In one process: the device call;
isim_service_timeline_device over the same spans (one pass over 64 B per span);
the DES step that wrote the spans; and the pinned device-to-host copy of the
spans (through one pinned buffer of --pinned-mib) followed by the host's table
(isim_service_quantiles_host, once; with --numpy also by numpy's lexsort,
once), which is what a host-side route pays.  The
device table is compared with the host's, word for word, before its time is
accepted.  No ratio is fixed in advance.

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
sys.path[:0] = [ROOT, os.path.join(ROOT, "istio-isotope_amd")]


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graph", choices=["c5p", "tree13"], default="c5p")
    ap.add_argument("--log2n", type=int, default=19, help="traces of the DES step")
    ap.add_argument("--mean-ns", type=int, default=None, help="mean gap (default: bench.py's 6 ms for c5p, 700 us for tree13)")
    ap.add_argument("--q", default="0.5,0.9,0.99,0.999")
    ap.add_argument("--pinned-mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the host table (and with it the comparison)")
    ap.add_argument("--numpy", action="store_true", help="also time the numpy route on the copied spans, once")
    ap.add_argument("--key", default=None, help="the name the result is stored under (default: the graph's); for a "
                    "library variant chosen with ISIM_LIB")
    ap.add_argument("--calls-only", type=int, default=0, metavar="N", help="tap the batch, make N device calls and "
                    "leave: the process a kernel trace is taken of (run with --worker, nothing is written)")
    ap.add_argument("--timeout", type=int, default=900, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "service_quantiles_bench.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def tree13():
    from isim.generators import tree_topology
    from isim.yamljson import obj_to_json
    t = tree_topology(3, 3)
    for s in t["services"]:
        s["script"] = [{"sleep": "1ms"}] + s.get("script", [])
    return obj_to_json(t)


def numpy_table(spans, n_services, ppm):
    """The table by numpy alone: per measure one lexsort by (service, value) for the class of all and one by
    (service, code, value) for the two codes, then the nearest ranks picked by index."""
    import numpy as np
    a, s, f = spans["arrival_ns"], spans["start_ns"], spans["finish_ns"]
    ok = (spans["service"] < n_services) & (a <= s) & (s <= f)
    a, s, f = a[ok], s[ok], f[ok]
    svc = spans["service"][ok].astype(np.int64)
    code = (spans["status"][ok] & 1).astype(np.int64)
    ow = 1 + len(ppm)
    out = np.zeros((n_services, 3, 3, ow), np.uint64)
    ppm = np.asarray(ppm, np.uint64)
    for c, key, n_keys in ((0, svc, n_services), (1, svc * 2 + code, 2 * n_services)):
        cnt = np.bincount(key, minlength=n_keys).astype(np.uint64)
        begin = np.cumsum(cnt) - cnt
        if c:   # [service][code] -> classes 1 and 2
            cnt, begin = cnt.reshape(n_services, 2), begin.reshape(n_services, 2)
        rank = np.maximum((cnt[..., None] * ppm + np.uint64(999_999)) // np.uint64(1_000_000), np.uint64(1))
        pick = np.minimum(begin[..., None] + rank - np.uint64(1), np.uint64(max(len(key) - 1, 0))).astype(np.int64)
        for m, v in enumerate((s - a, f - s, f - a)):
            sv = v[np.lexsort((v, key))] if len(v) else np.zeros(1, np.uint64)
            got = np.where(cnt[..., None] > 0, sv[pick], np.uint64(0))
            if c:
                out[:, m, 1:, 0], out[:, m, 1:, 1:] = cnt, got
            else:
                out[:, m, 0, 0], out[:, m, 0, 1:] = cnt, got
    return np.concatenate([out.ravel(), np.array([int(ok.sum()), int((~ok).sum())], np.uint64)])


def worker(a):
    import numpy as np
    import torch

    import bench
    import isim
    from isim import native
    from isim.des_spans import make_tap
    from isim.service_quantiles import (service_quantiles_device, service_quantiles_table_words,
                                        service_quantiles_workspace_bytes)
    from isim.service_timeline import (service_timeline_device, service_timeline_table_words,
                                       service_timeline_workspace_bytes)

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
    tap = make_tap(0, 0, native.Q_ALL, n, cap, ids.data_ptr(), off.data_ptr(), spans.data_ptr(), info.data_ptr())

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

    t_des = timed(lambda: call(tap), warmup=1, reps=3)
    word = info.cpu().numpy().view(np.uint64)
    total = int(word[native.SPAN_TOTAL])
    assert int(word[native.SPAN_WRITTEN]) == n == int(word[native.DES_SPAN_MATCHES]) and total <= cap

    words = service_quantiles_table_words(h, len(q))
    qws_bytes = service_quantiles_workspace_bytes(h, cap, len(q))
    out = torch.full((words,), -1, dtype=torch.int64, device=dev)
    qws = torch.empty(qws_bytes + 8, dtype=torch.uint8, device=dev)

    def select():
        service_quantiles_device(h, q, off.data_ptr(), spans.data_ptr(), cap, info.data_ptr(), out.data_ptr(),
                                 qws.data_ptr(), qws_bytes, stream)

    select()
    torch.cuda.synchronize()
    dev_table = out.cpu().numpy().view(np.uint64).copy()
    if a.calls_only:
        for _ in range(a.calls_only):
            select()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), dev_table)
        return

    chunk = min(total * 64, a.pinned_mib << 20)
    pinned = torch.empty(chunk, dtype=torch.uint8).pin_memory()

    def copy():
        for lo in range(0, total * 64, chunk):
            hi = min(total * 64, lo + chunk)
            pinned[:hi - lo].copy_(spans[lo:hi], non_blocking=True)

    t_copy = timed(copy, warmup=1, reps=5)
    host = None
    if not a.no_host:
        h_spans = spans.cpu().numpy().view(isim.DES_SPAN_DTYPE)[:total]
        t0 = time.perf_counter()
        host_table = isim.service_quantiles_host(h, h_spans, q)
        host = {"host_table_s": time.perf_counter() - t0}
        bad = np.flatnonzero(host_table != dev_table)
        assert bad.size == 0, (bad[:4], host_table[bad[:4]], dev_table[bad[:4]])
        if a.numpy:
            t0 = time.perf_counter()
            np_table = numpy_table(h_spans, int(h.info.n_services), isim.quantiles.q_to_ppm(q))
            host["numpy_table_s"] = time.perf_counter() - t0
            assert np.array_equal(np_table, dev_table)
        del h_spans
    t_sel = timed(select)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), dev_table)     # every timed call wrote the same table

    window, n_windows = 1_000_000, 1024
    twords = service_timeline_table_words(h, window, n_windows, 0)
    tws_bytes = service_timeline_workspace_bytes(h, window, n_windows, 0)
    tout, tws = i64(twords), torch.empty(tws_bytes, dtype=torch.uint8, device=dev)
    t_fold = timed(lambda: service_timeline_device(h, window, n_windows, 0, off.data_ptr(), spans.data_ptr(), cap,
                                                   info.data_ptr(), tout.data_ptr(), tws.data_ptr(), tws_bytes, stream))

    seg = np.sort(dev_table[:-2].reshape(-1, 3, 3, 1 + len(q))[:, 0, 0, 0])
    res = {"device": torch.cuda.get_device_name(0), "n_traces": n, "mean_ns": mean, "q": list(q),
           "n_services": int(h.info.n_services), "spans": total, "span_bytes": total * 64,
           "segments": {"long": int((seg > native.SVQ_STAGE).sum()), "short": int(((seg > 0) & (seg <= native.SVQ_STAGE)).sum()),
                        "empty": int((seg == 0).sum()), "median": int(seg[len(seg) // 2]), "max": int(seg[-1])},
           "workspace_bytes": int(qws_bytes), "table_words": int(words), "library": os.path.basename(native.LIB_PATH),
           "service_quantiles_device": dict(t_sel, ns_per_span=1e6 * t_sel["median_ms"] / max(1, total)),
           "service_timeline_device_1ms": t_fold, "des_step_with_tap": t_des,
           "pinned_copy": dict(t_copy, pinned_buffer_bytes=int(chunk),
                               bytes_per_s=total * 64 / (1e-3 * t_copy["median_ms"])),
           "host": host, "compared_with_host": host is not None,
           "select_over_copy": t_sel["median_ms"] / t_copy["median_ms"],
           "select_over_timeline_fold": t_sel["median_ms"] / t_fold["median_ms"],
           "select_over_des_step": t_sel["median_ms"] / t_des["median_ms"]}
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
        print(f"service_quantiles_bench: the measuring process passed its limit of {a.timeout} s", file=sys.stderr)
        rc = 124
    sys.exit(rc)


if __name__ == "__main__":
    main()
