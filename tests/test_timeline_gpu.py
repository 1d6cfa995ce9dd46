"""The load-test timeline on the GPU: isim_des_arrivals*
against a numpy restatement of the Philox draw and the fixed-point
exponential, and against the engine itself (the Lindley recursion of a
one-service graph); isim_timeline* against numpy over rows computed with
Python integers.  Every comparison is equality of integers."""
import json
import os

import numpy as np
import pytest

import isim
from isim import native
from isim.yamljson import yaml_to_json
from oracle import des as od
from oracle import philox as op

from conftest import TOPOLOGIES
from test_quantiles_gpu import peel_lanes

pytestmark = pytest.mark.gpu

U64 = np.uint64
M32 = U64(0xFFFFFFFF)
MAXU = (1 << 64) - 1
W = native.TL_ROW_WORDS
BIT31 = np.uint32(1 << 31)
CHUNK = 8192  # traces per arrivals chunk


# ---- the restatement: Philox4x32-10, the Q24 exponential, the prefix sum
def philox_np(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over u64 arrays holding 32-bit words; returns the four output words."""
    c0, c1, c2, c3 = (np.asarray(x, U64) & M32 for x in (c0, c1, c2, c3))
    k0, k1 = U64(k0 & 0xFFFFFFFF), U64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0 = U64(op.M0) * c0
        p1 = U64(op.M1) * c2
        c0, c1, c2, c3 = (p1 >> U64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> U64(32)) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + U64(op.W0)) & M32
        k1 = (k1 + U64(op.W1)) & M32
    return c0, c1, c2, c3


def _ln_table():
    import math
    return np.array([round(math.log1p(i / 256.0) * 16777216.0) for i in range(257)], np.int64)


def exp_q24_np(u):
    """oracle.des.exp_q24_py's table arithmetic over an array of u32 draws."""
    tab = _ln_table()
    w = (np.asarray(u, np.int64) >> 8) + 1
    e = np.floor(np.log2(w.astype(np.float64))).astype(np.int64)  # w <= 2^24: exact in doubles
    e = np.where((np.int64(1) << e) > w, e - 1, e)
    e = np.where((np.int64(2) << e) <= w, e + 1, e)
    f = (w << (24 - e)) & 0xFFFFFF
    idx, rem = f >> 16, f & 0xFFFF
    lnm = tab[idx] + (((tab[idx + 1] - tab[idx]) * rem) >> 16)
    return (24 * 11629080 - (e * 11629080 + lnm)).astype(U64)


def arrivals_np(seed, mean, trace_begin, n):
    t = (np.arange(n, dtype=U64) + U64(trace_begin))
    u = philox_np(t & M32, t >> U64(32), 0, 0x80000001, seed & 0xFFFFFFFF, seed >> 32)[0]
    gap = (U64(mean) * exp_q24_np(u)) >> U64(24)   # mean <= 2^34, E < 2^29: below 2^63
    return np.cumsum(gap, dtype=U64)


def test_restatement_is_the_oracles():
    rng = np.random.default_rng(1)
    ctr = rng.integers(0, 1 << 32, (6, 4), dtype=np.uint64)
    ctr[0] = [0, 0, 0, 0]
    ctr[1] = [0xFFFFFFFF, 0xFFFFFFFF, 0, 0x80000001]
    key = (0x12345678, 0x9ABCDEF0)
    got = np.stack(philox_np(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], *key), axis=1)
    for i in range(len(ctr)):
        assert tuple(int(x) for x in got[i]) == op.philox4x32_10([int(x) for x in ctr[i]], key)
    us = np.array([0, 1, 255, 256, 257, 0xFFFFFFFF, 0xFFFFFF00, 0x80000000, 0x7FFFFFFF, 12345678] +
                  rng.integers(0, 1 << 32, 200).tolist(), np.int64)
    assert exp_q24_np(us).tolist() == [od.exp_q24_py(int(u)) for u in us]


def _doc(sleep="1ms"):
    return {"services": [{"name": "a", "isEntrypoint": True, "script": [{"sleep": sleep}]}]}


@pytest.fixture(scope="module")
def handler():
    return isim.Handler(isim.ServiceGraph.from_json(json.dumps(_doc())), None, isim.SimParams(seed=0x5EED0123456789AB))


@pytest.mark.parametrize("n", [1, 63, 64, 8191, 8192, 8193, 70_001])
@pytest.mark.parametrize("mean", [1, 1 << 34])
@pytest.mark.parametrize("begin", [0, (1 << 32) - 5])
def test_arrivals_against_restatement(gpu, handler, n, mean, begin):
    got = isim.des_arrivals(handler, mean, begin, n)
    want = arrivals_np(handler.params.seed, mean, begin, n)
    assert got.dtype == np.uint64 and np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()


def test_arrivals_other_seed_and_mean(gpu):
    """Nothing but the seed, the mean and the trace ids enters: a graph outside the one above, the default seed."""
    h = isim.handler_from_service_graph_yaml(os.path.join(TOPOLOGIES, "canonical.yaml"))
    got = isim.des_arrivals(h, 6_000_000, 777, 5000)
    assert np.array_equal(got, arrivals_np(h.params.seed, 6_000_000, 777, 5000))
    assert (np.diff(got.astype(np.int64)) >= 0).all() and got[-1] > 5000 * 5_000_000


def test_arrivals_past_one_scan_block(gpu, handler):
    """More than 1024 chunks, so the scan of the chunk sums takes a second
    tier: sampled positions and every chunk edge against the small path
    (pinned above) through A[k + j] - A[k - 1] == arrivals(trace_begin + k, 64)[j]."""
    n, mean, begin = CHUNK * 1024 + 8193, 1000, 12345
    big = isim.des_arrivals(handler, mean, begin, n)
    assert np.array_equal(big[:70_001], arrivals_np(handler.params.seed, mean, begin, 70_001))
    gaps = np.diff(big.astype(np.int64))
    assert (gaps >= 0).all()
    # every chunk edge: the gap across it is the restated gap of that trace
    edges = np.arange(CHUNK, n, CHUNK)
    t = edges.astype(U64) + U64(begin)
    u = philox_np(t & M32, t >> U64(32), 0, 0x80000001, handler.params.seed & 0xFFFFFFFF, handler.params.seed >> 32)[0]
    assert np.array_equal(big[edges] - big[edges - 1], (U64(mean) * exp_q24_np(u)) >> U64(24))
    rng = np.random.default_rng(3)
    ks = sorted(set(rng.integers(1, n - 64, 12).tolist() + [CHUNK * 1023 - 1, CHUNK * 1024 - 32, CHUNK * 1024, n - 64]))
    checked = 0
    for k in ks:
        small = isim.des_arrivals(handler, mean, begin + k, 64)
        assert np.array_equal(big[k:k + 64] - big[k - 1], small), k
        checked += 64
    assert checked >= 1000


@pytest.mark.parametrize("begin", [0, 1_000_003])
def test_arrivals_are_the_engines(gpu, begin):
    """One service, one replica, one sleep P: the Lindley recursion over the
    exported arrivals, S_t = max(A_t, S_{t-1} + P), gives isim_serve_des's
    latency S_t + P - A_t for every trace."""
    P, n = 1_000_000, 20_000
    h = isim.Handler(isim.ServiceGraph.from_json(json.dumps(_doc("1ms"))), None, isim.SimParams())
    d = isim.DesHandler(h, 1_200_000)
    recs, _, _ = d.serve(begin, n, device=0)
    A = d.arrivals(begin, n).astype(np.int64)
    t = np.arange(n, dtype=np.int64)
    S = t * P + np.maximum.accumulate(A - t * P)   # S_t = max(A_t, S_{t-1} + P), an idle start
    want = (S + P - A).astype(U64)
    assert np.array_equal(recs["latency_ns"], want), np.argwhere(recs["latency_ns"] != want)[:4].tolist()
    assert (want > P).sum() > n // 10   # the queue does form


# ---- the timeline against numpy
def rows_of(x, t0, window, n_windows):
    """Row per time, in Python integers (object arrays)."""
    x = np.asarray(x, U64).astype(object)
    w = (x - t0) // window
    return np.where(x < t0, 0, 1 + np.minimum(w, n_windows)).astype(np.int64)


def prom_bucket(lat):
    """The stats buffer's histogram: the first edge (whole ms) >= the latency; 32: above 500 ms."""
    edges = np.array(PROM_MS, np.int64)
    return np.searchsorted(edges * 1_000_000, np.minimum(np.asarray(lat, U64), U64(1 << 62)).astype(np.int64),
                           side="left")


# prometheus/handler.go:26-35, as include/isim.h lists them for ISIM_ST_PROM
PROM_MS = [7, 8, 9, 10, 11, 12, 14, 16, 18, 20, 25, 30, 35, 40, 45, 50, 60, 70, 80, 90, 100, 120, 140, 160, 180,
           200, 250, 300, 350, 400, 450, 500]


def expect(arr, recs, t0, window, n_windows):
    arr = np.asarray(arr, U64)
    lat = recs["latency_ns"].astype(U64)
    c = arr + lat
    c = np.where(c < arr, U64(MAXU), c)  # saturates
    ra, rc = rows_of(arr, t0, window, n_windows), rows_of(c, t0, window, n_windows)
    code = ((recs["status_err"] & BIT31) != 0).astype(np.int64)
    out = np.zeros((n_windows + 2, W), U64)
    np.add.at(out, (ra, native.TL_ARRIVED), U64(1))
    np.add.at(out, (rc, native.TL_DONE + code), U64(1))
    np.add.at(out, (rc, native.TL_SUM_LAT + code), lat)
    np.maximum.at(out, (rc, native.TL_MAX_LAT + code), lat)
    np.add.at(out, (rc, native.TL_PROM + code * native.N_PROM + prom_bucket(lat)), U64(1))
    return out.reshape(-1)


def make_recs(lat, seed):
    rng = np.random.default_rng(seed)
    recs = np.zeros(len(lat), isim.REC_DTYPE)
    recs["latency_ns"] = lat
    recs["hops"] = rng.integers(0, 1 << 32, len(lat), dtype=np.uint64).astype(np.uint32)
    low = rng.integers(0, 1 << 31, len(lat), dtype=np.uint64).astype(np.uint32)
    recs["status_err"] = low | np.where(rng.integers(0, 2, len(lat)).astype(bool), BIT31, np.uint32(0))
    return recs


def test_prom_restatement():
    assert [round(x * 1000) for x in isim.prometheus.DURATION_BUCKETS] == PROM_MS
    assert prom_bucket([0, 7_000_000, 7_000_001, 500_000_000, 500_000_001, MAXU]).tolist() == [0, 0, 1, 31, 32, 32]
    assert len(PROM_MS) == native.N_PROM - 1


def make_case(n, window, n_windows, t0_mode, seed):
    """Ascending arrivals over about 1.25 times the windows (at most 5000 of
    them); latencies that complete in the same window, the next one, thousands
    later and after the last; the forced values of the issue."""
    rng = np.random.default_rng(seed)
    span = min(max(window * min(n_windows, 5000) * 5 // 4, 1000), 1 << 62)
    arr = np.sort(rng.integers(0, span, n, dtype=np.uint64))
    t0 = 0 if t0_mode == 0 or n == 0 else int(arr[n // 3])
    kinds = rng.integers(0, 6, n)
    lat = np.zeros(n, object)
    small = [int(x) for x in rng.integers(0, max(2, min(window, 1 << 62)), n, dtype=np.uint64)]
    for i in range(n):
        k = kinds[i]
        lat[i] = (small[i] // 2 if k == 0 else                       # mostly the same window
                  min(window, MAXU) if k == 1 else                    # the next one
                  min(window * 3000 + small[i], MAXU) if k == 2 else  # thousands later (or after)
                  MAXU - small[i] if k == 3 else                      # saturates or lands after
                  (0, 7_000_000, 7_000_001, 500_000_000, 500_000_001)[small[i] % 5] if k == 4 else
                  small[i])
    lat = np.array([int(x) for x in lat], U64) if n else np.zeros(0, U64)
    if n >= 8:
        k = min(3, n_windows)
        forced_a = [t0, min(t0 + k * window, MAXU), min(t0 + k * window, MAXU) - 1, max(1, t0), t0 + 1 if t0 < MAXU else t0]
        forced_l = [0, 7_000_000, 7_000_001, MAXU, 500_000_001]
        pos = rng.permutation(n)[:len(forced_a)]
        arr[pos] = np.array(forced_a, U64)
        lat[pos] = np.array(forced_l, U64)
        order = np.argsort(arr, kind="stable")
        arr, lat = arr[order], lat[order]
    return arr, make_recs(lat, seed + 1), t0


WINDOWS = [(1, 1), (1, 4096), (7, 37), (10**6, 2), (1 << 40, 65536), (MAXU, 1)]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 70_001])
@pytest.mark.parametrize("window,n_windows", WINDOWS)
def test_timeline_against_numpy(gpu, n, window, n_windows):
    for t0_mode in (0, 1):
        arr, recs, t0 = make_case(n, window, n_windows, t0_mode, seed=n * 7 + n_windows + t0_mode)
        for permuted in (False, True):
            if permuted:
                p = np.random.default_rng(n).permutation(n)
                arr, recs = arr[p], recs[p]
            got = isim.timeline_table(arr, recs, window, n_windows, t0)
            want = expect(arr, recs, t0, window, n_windows)
            bad = np.argwhere(got != want)
            assert bad.size == 0, (t0_mode, permuted, [(int(i) // W, int(i) % W, int(got[i]), int(want[i]))
                                                        for i in bad[:4, 0]])
            t = got.reshape(-1, W)
            assert int(t[:, native.TL_ARRIVED].sum()) == n
            assert int(t[:, native.TL_DONE:native.TL_DONE + 2].sum()) == n == int(t[:, native.TL_PROM:].sum())
            if t0_mode == 1 and n >= 8:
                assert t[0, native.TL_ARRIVED] > 0   # the "before" row fills


@pytest.mark.parametrize("n", [64, 320, 5000])
def test_all_lanes_one_word(gpu, n):
    arr = np.full(n, 123_456_789, U64)
    recs = np.zeros(n, isim.REC_DTYPE)
    recs["latency_ns"] = 8_000_000
    got = isim.timeline_table(arr, recs, 10**6, 200, 0)
    assert np.array_equal(got, expect(arr, recs, 0, 10**6, 200))
    t = got.reshape(-1, W)
    assert t[124, native.TL_ARRIVED] == n and t[132, native.TL_DONE] == n and t[132, native.TL_SUM_LAT] == n * 8_000_000
    assert t[132, native.TL_MAX_LAT] == 8_000_000 and t[132, native.TL_PROM + 1] == n


def peel_case(reverse):
    """One wave (test_quantiles_gpu.peel_lanes: slot values held by 51, 1, 3, 4 and 5 lanes), every record a
    200: arrivals in window `slot`, latencies of 8.5 ms + 2 ms * slot (five Prometheus buckets)."""
    lanes = peel_lanes()[::-1] if reverse else peel_lanes()
    recs = make_recs(U64(8_500_000) + lanes * U64(2_000_000), 31)
    recs["status_err"] &= ~BIT31
    return lanes * U64(1_000_000) + U64(5), recs


def test_peel_threshold(gpu):
    """Multiplicities on both sides of the peel's 'fewer than four' break (csrc/wave_peel.h), in lane order
    and reversed: in the arrival rows and the histogram words with every completion in the 'after' row of 8
    windows of 1 ms, then in the completion rows too (one arrival time, 30 windows)."""
    for reverse in (False, True):
        arr, recs = peel_case(reverse)
        got = isim.timeline_table(arr, recs, 10**6, 8, 0)
        assert np.array_equal(got, expect(arr, recs, 0, 10**6, 8)), reverse
        t = got.reshape(-1, W)
        assert t[1:7, native.TL_ARRIVED].tolist() == [51, 1, 0, 3, 4, 5] and t[9, native.TL_DONE] == 64
        arr[:] = 5
        got = isim.timeline_table(arr, recs, 10**6, 30, 0)
        assert np.array_equal(got, expect(arr, recs, 0, 10**6, 30)), reverse
        assert sorted(got.reshape(-1, W)[:, native.TL_DONE].tolist())[-5:] == [1, 3, 4, 5, 51]


@pytest.mark.parametrize("window,n_windows", [(1000, 64), (1 << 20, 1000), (999, 65536)])
def test_all_lanes_different_rows(gpu, window, n_windows):
    """Each wave's 64 lanes in 64 different rows, arrivals and completions: rows 1000 apart where there are enough."""
    step = max(1, (n_windows // 64)) * window
    arr = (np.arange(640, dtype=U64) % U64(64)) * U64(step)
    recs = make_recs(np.zeros(640, U64), 5)
    got = isim.timeline_table(arr, recs, window, n_windows, 0)
    assert np.array_equal(got, expect(arr, recs, 0, window, n_windows))
    assert (got.reshape(-1, W)[:, native.TL_ARRIVED] == 10).sum() == 64


def _upload(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(torch.device("cuda", 0))


def test_accumulation(gpu):
    """Two device calls into one table = the host merge of two single tables = one call over the concatenation."""
    import torch
    window, n_windows = 10**6, 300
    a1, r1, _ = make_case(9000, window, n_windows, 0, seed=21)
    a2, r2, _ = make_case(4001, window, n_windows, 0, seed=22)
    t1 = isim.timeline_table(a1, r1, window, n_windows)
    t2 = isim.timeline_table(a2, r2, window, n_windows)
    merged = isim.timeline_merge(n_windows, t1.copy(), t2)
    both = isim.timeline_table(np.concatenate([a1, a2]), np.concatenate([r1, r2]), window, n_windows)
    assert np.array_equal(merged, both)
    assert np.array_equal(both, expect(np.concatenate([a1, a2]), np.concatenate([r1, r2]), 0, window, n_windows))
    out = torch.zeros(isim.timeline_out_words(n_windows), dtype=torch.int64, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    for a, r in ((a1, r1), (a2, r2)):
        da, dr = _upload(torch, a), _upload(torch, r)
        isim.timeline_device(da.data_ptr(), dr.data_ptr(), len(a), window, n_windows, d_out=out.data_ptr(), stream=s)
        torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(U64), both)
    # the host convenience accumulates as well
    assert np.array_equal(isim.timeline_table(a2, r2, window, n_windows, out=t1.copy()), both)


def test_dirty_workspace_and_capture(gpu, handler):
    """Arrivals with a 0xA5-filled workspace; then arrivals and the timeline
    captured as one chain, with nothing run before the capture.  A capture
    records without running, so the table is compared after one replay (the
    single result) and after three (its sums three times, its maxima once)."""
    import torch
    n, mean, begin, window, n_windows = 20_000, 50_000, 99, 10**7, 120
    dev = torch.device("cuda", 0)
    wsb = isim.des_arrivals_workspace_bytes(n)
    ws = torch.full((wsb,), 0xA5, dtype=torch.uint8, device=dev)
    d_arr = torch.full((n,), -1, dtype=torch.int64, device=dev)
    want_arr = arrivals_np(handler.params.seed, mean, begin, n)
    recs = make_recs(np.random.default_rng(4).integers(0, 4 * 10**7, n, dtype=np.uint64), 6)
    d_rec = _upload(torch, recs)
    out = torch.zeros(isim.timeline_out_words(n_windows), dtype=torch.int64, device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        s = torch.cuda.current_stream().cuda_stream
        isim.des_arrivals_device(handler, mean, begin, n, d_arrivals=d_arr.data_ptr(), d_workspace=ws.data_ptr(),
                                 workspace_bytes=wsb, stream=s)
        isim.timeline_device(d_arr.data_ptr(), d_rec.data_ptr(), n, window, n_windows, d_out=out.data_ptr(), stream=s)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(d_arr.cpu().numpy().view(U64), want_arr)
    single = expect(want_arr, recs, 0, window, n_windows)
    assert np.array_equal(out.cpu().numpy().view(U64), single)
    ws.fill_(0x5A)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    three = single.reshape(-1, W) * U64(3)
    three[:, native.TL_MAX_LAT:native.TL_MAX_LAT + 2] = single.reshape(-1, W)[:, native.TL_MAX_LAT:native.TL_MAX_LAT + 2]
    assert np.array_equal(out.cpu().numpy().view(U64), three.reshape(-1))


def test_end_to_end_des(gpu):
    """DesHandler.timeline on the committed 13-service tree with a 2 ms sleep
    in every service, at a 1 ms mean gap (overloaded: the queue grows)."""
    doc = json.loads(yaml_to_json(open(os.path.join(TOPOLOGIES, "tree-13-services.yaml"), "rb").read()))
    for s in doc["services"]:
        s["script"] = [{"sleep": "2ms"}] + (s.get("script") or [])
        s["errorRate"] = 0.05
    h = isim.Handler(isim.ServiceGraph.from_json(json.dumps(doc)), None, isim.SimParams())
    d = isim.DesHandler(h, 1_000_000)
    n, begin, window, n_windows = 6000, 17, 250_000_000, 20
    tl = d.timeline(begin, n, window, n_windows)
    recs, _, _ = d.serve(begin, n)
    arr = d.arrivals(begin, n)
    want = isim.decode_timeline(expect(arr, recs, 0, window, n_windows), n_windows, 0, window)
    for k in ("arrived", "done", "sum_latency_ns", "max_latency_ns", "prom", "in_flight_end"):
        assert np.array_equal(tl[k], want[k]), k
    for k in ("arrived", "done", "prom"):
        assert np.array_equal(tl["after"][k], want["after"][k]) and not tl["before"][k].any(), k
    assert int(tl["arrived"].sum() + tl["after"]["arrived"]) == n
    # every trace: in flight when the last window ends, or arriving later, completes in "after"
    assert int(tl["in_flight_end"][-1]) + int(tl["after"]["arrived"]) == int(tl["after"]["done"].sum())
    assert int(tl["done"].sum() + tl["after"]["done"].sum()) == n
    # overloaded: the backlog grows and so does the latency of what completes
    assert tl["in_flight_end"][-1] > tl["in_flight_end"][n_windows // 2] > tl["in_flight_end"][1] > 0
    assert tl["done"][1].sum() > 0
