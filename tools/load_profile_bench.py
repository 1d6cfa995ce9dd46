"""Timing of arrivals under a load profile (isim_profile_arrivals_device,
DESIGN.md §17) against the constant-mean arrivals of the same handler and batch
(isim_des_arrivals_device, the code every earlier release has), and of a
config-5 DES step under a one-segment profile against the same step through
isim_serve_des_device.

Arrivals: 2^24 traces, profiles of 1, 16 and 1024 segments sized so that the
batch crosses all of them, Poisson and paced.  Each call is timed with HIP
events (--warmup calls, then --reps: median, min and max).  Writes a JSON
(--out) with the times and the ratio profile / constant.

The parent process never opens the GPU: it starts the measuring process under
a time limit (--timeout) and reports its exit status.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "istio-isotope_amd")]

MEAN_NS = 6_000_000
SEGMENTS = (1, 16, 1024)


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2n", type=int, default=24, help="traces of the arrivals batch")
    ap.add_argument("--des-log2n", type=int, default=20, help="traces of the config-5 DES step")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=540, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "load_profile_bench.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def profile_of(isim, k, n, paced):
    """k segments the n-trace batch crosses, means alternating between MEAN_NS and 3/4 of it: each of the
    first k - 1 lasts as long as n / k arrivals take at the shorter mean, so at most n / k traces fall in it."""
    if k == 1:
        return isim.LoadProfile.constant(MEAN_NS, paced=paced)
    share = n * (MEAN_NS * 3 // 4) // k
    return isim.LoadProfile.steps([(share, MEAN_NS * 3 // 4 if j % 2 else MEAN_NS) for j in range(k - 1)], MEAN_NS,
                                  paced=paced)


def worker(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("load_profile_bench needs a GPU: it measures, it does not fall back")
    import bench
    import isim
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return ms

    n = 1 << args.log2n
    h = isim.Handler(isim.ServiceGraph.from_json('{"services":[{"name":"a","isEntrypoint":true}]}'), None,
                     isim.SimParams())
    arr = torch.empty(n, dtype=torch.int64, device=dev)
    wsb = max(isim.profile_arrivals_workspace_bytes(n), isim.des_arrivals_workspace_bytes(n))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    base = timed(lambda: isim.des_arrivals_device(h, MEAN_NS, 0, n, d_arrivals=arr.data_ptr(),
                                                  d_workspace=ws.data_ptr(), workspace_bytes=wsb,
                                                  stream=stream.cuda_stream))
    entries = []
    for paced in (False, True):
        for k in SEGMENTS:
            p = profile_of(isim, k, n, paced)
            ms = timed(lambda: isim.profile_arrivals_device(h, p, 0, n, d_arrivals=arr.data_ptr(),
                                                            d_workspace=ws.data_ptr(), workspace_bytes=wsb,
                                                            stream=stream.cuda_stream))
            torch.cuda.synchronize()
            last = int(arr[-1].item())
            e = {"what": "arrivals", "n_traces": n, "segments": k, "paced": paced, "profile": spread(ms),
                 "constant": spread(base), "profile_over_constant": statistics.median(ms) / statistics.median(base),
                 "last_arrival_ns": last, "last_segment_reached": bool(last >= sum(d for d, _ in p.segments))}
            print(json.dumps(e), flush=True)
            entries.append(e)

    # a config-5 DES step: the same batch under the constant mean and under a one-segment profile
    nd = 1 << args.des_log2n
    j, _ = bench.build_graph("c5")
    hd = isim.Handler(isim.ServiceGraph.from_json(j), None, isim.SimParams(error_mode=isim.MODE_A))
    dc, dp = isim.DesHandler(hd, MEAN_NS), isim.DesHandler(hd, profile=isim.LoadProfile.constant(MEAN_NS))
    wsb = dc.workspace_bytes(nd)
    stats = torch.zeros(hd.info.stats_words, dtype=torch.int64, device=dev)
    recs = torch.empty((nd, 2), dtype=torch.int64, device=dev)
    table = torch.zeros(max(1, dc.table_words), dtype=torch.int64, device=dev)
    wsd = torch.empty(wsb // 8 + 1, dtype=torch.int64, device=dev)

    def step(d):
        return lambda: d.serve_device(0, nd, recs.data_ptr(), stats.data_ptr(), table.data_ptr(), wsd.data_ptr(), wsb,
                                      stream.cuda_stream)

    c_ms, p_ms = timed(step(dc)), timed(step(dp))
    retries = int(stats[isim.native.ST_DES_RETRY].item())
    e = {"what": "c5 DES step", "n_traces": nd, "segments": 1, "paced": False, "profile": spread(p_ms),
         "constant": spread(c_ms), "profile_over_constant": statistics.median(p_ms) / statistics.median(c_ms),
         "batches_not_accumulated": retries}
    print(json.dumps(e), flush=True)
    entries.append(e)
    res = {"device": torch.cuda.get_device_name(dev), "warmup": args.warmup, "timing": "HIP events around one call",
           "entries": entries}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


def main():
    args = parse()
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
