"""Closed-loop clients on the GPU: isim_closed_loop* against
isim_closed_loop_host value for value in both regimes of the kernels, a large
batch against the per-connection closed form in numpy, chaining and graph
capture on the device, the timeline of a served walk under 64 connections, and
ClosedLoopRun against a host replay."""
import json

import numpy as np
import pytest

import isim
from isim import native
from isim.generators import config3p_topology
from isim.yamljson import obj_to_json

pytestmark = pytest.mark.gpu

U64 = np.uint64
TOP = (1 << 64) - 1
MEAN = 1 << 19      # of latencies random below 2^20
PERIODS = (0, 5_000, 10_000_000, 500_000)      # max; far below the mean; far above the maximum; near the mean


def records(lat):
    r = np.zeros(len(lat), isim.REC_DTYPE)
    r["latency_ns"] = lat
    return r


def latencies(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "zero":
        return np.zeros(n, U64)
    lat = rng.integers(0, 1 << 20, n, dtype=np.uint64)
    if kind == "huge" and n:
        at = rng.integers(0, n, max(1, n // 1000))
        lat[at] = np.where(rng.random(len(at)) < 0.5, U64(1 << 63), U64(TOP))
    return lat


def multi_block_n(C_):
    """The smallest n (+ 5) at which a thread of the composite scan (csrc/closed_loop.hip cl_scan_states) owns
    more than one row block.  Staged regime (C < 64): row blocks of (256 // C) * 16 rows, 1024 // C scan threads
    per connection.  Direct regime: row blocks of 16 rows at these sizes, 1024 // C scan threads per connection
    below 1024 connections and one at or above."""
    if C_ < 64:
        return (1024 // C_) * (256 // C_) * 16 * C_ + 5
    return 16 * (1024 // C_ + 1) * C_ + 5 if C_ < 1024 else 2 * 16 * C_ + 5


def check(cl, rec, first, state, what):
    want = cl.arrivals_host(rec, first, state)
    got = cl.arrivals(rec, first, state)
    for name, g, w in zip(("arrivals", "free_at", "info"), got, want):
        assert g.dtype == U64 and np.array_equal(g, w), (what, name, np.argwhere(g != w)[:4].tolist())
    return got


# ---- 1. the device against the host function
@pytest.mark.parametrize("C_", [1, 2, 3, 4, 63, 64, 65, 100, 256, 1000, 65536])
def test_device_against_host(gpu, C_):
    big = multi_block_n(C_)
    scan_threads = 1024 // C_ if C_ < 1024 else 1
    assert isim.closed_loop_workspace_bytes(big, C_) // (16 * C_) > scan_threads      # row blocks per connection
    sizes = sorted({1, C_ - 1, C_, C_ + 1, 8191, 8192, 8193, 3 * 8192 + 5})
    rng = np.random.default_rng(C_)
    combo = 0
    for n in sizes + [big]:
        lats = {kind: records(latencies(kind, n, 31 * C_ + n % 1000)) for kind in ("random", "zero", "huge")}
        for p in PERIODS:
            for kind, rec in lats.items():
                # first_index, uniform and the state: all eight combinations in turn
                first = (0, 7 * C_ + C_ // 2 + 1)[combo & 1]
                uniform, with_state = bool(combo & 2), bool(combo & 4)
                combo += 1
                if n == big and kind == "zero" and p in PERIODS[1:3]:
                    continue      # the large size: each period and each kind, not every pair
                state = rng.integers(0, 1 << 22, C_, dtype=np.uint64) if with_state else None
                cl = isim.ClosedLoop(C_, period_ns=p, uniform=uniform)
                a, f, info = check(cl, rec, first, state, (C_, n, p, kind, first, uniform, with_state))
                if n == 0:
                    assert info.tolist() == [int(f.max()), int(f.min()), 0, 0]
    assert combo >= 8 * 12


def test_null_state_is_zeros_in_nothing_out(gpu):
    """The device entry with a null d_free_at: the arrivals of a run from zeros, the info of that run."""
    import torch
    dev = torch.device("cuda", 0)
    for C_, n in ((4, 10_000), (100, 10_000)):
        cl = isim.ClosedLoop(C_, period_ns=300_000, uniform=True)
        rec = records(latencies("random", n, 1))
        want_a, _, want_i = cl.arrivals_host(rec, 3)
        d_rec = torch.from_numpy(rec.view(np.int64).copy()).to(dev)
        d_arr = torch.full((n,), -1, dtype=torch.int64, device=dev)
        d_info = torch.full((4,), -1, dtype=torch.int64, device=dev)
        ws = torch.empty(isim.closed_loop_workspace_bytes(n, C_), dtype=torch.uint8, device=dev)
        cl.arrivals_device(d_rec.data_ptr(), n, 3, d_free_at=0, d_arrivals=d_arr.data_ptr(), d_info=d_info.data_ptr(),
                           d_workspace=ws.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(d_arr.cpu().numpy().view(U64), want_a)
        assert np.array_equal(d_info.cpu().numpy().view(U64), want_i)


# ---- 2. a large batch against the closed form
def closed_form(C_, p, uniform, k0, lat, F_in):
    """Per connection, F_k = P_k + max(F_in, max_{j<=k}(s_j - P_{j-1})) and A_k = max(F_{k-1}, s_k), for a batch
    that starts at request k0 * C; nothing here saturates, so int64 holds every value."""
    n = len(lat)
    rows = -(-n // C_)
    L = np.zeros(rows * C_, np.int64)
    L[:n] = lat.astype(np.int64)
    L = L.reshape(rows, C_)
    c = np.arange(C_, dtype=np.int64)
    o = c * p // C_ if uniform else np.zeros(C_, np.int64)
    s = o[None, :] + (k0 + np.arange(rows, dtype=np.int64))[:, None] * p
    P = np.cumsum(L, axis=0)
    F = P + np.maximum(F_in.astype(np.int64)[None, :], np.maximum.accumulate(s - (P - L), axis=0))
    F_prev = np.vstack([F_in.astype(np.int64)[None, :], F[:-1]])
    A = np.maximum(F_prev, s)
    # the state after the batch: a connection's last real request (the padded tail has none in the last row)
    last_row = np.where(c < n - (rows - 1) * C_, rows - 1, rows - 2)
    return A.reshape(-1)[:n].astype(U64), F[last_row, c].astype(U64)


@pytest.mark.parametrize("C_", [64, 4])
def test_large_batch_against_closed_form(gpu, C_):
    n, k0 = (1 << 22) + 8192 + 3, 1000
    lat = latencies("random", n, 77)
    rec = records(lat)
    F_in = np.random.default_rng(8).integers(0, 1 << 24, C_, dtype=np.uint64)
    for p, uniform in ((0, False), (C_ * 100_000, True), (MEAN, True)):
        want_a, want_f = closed_form(C_, p, uniform, k0, lat, F_in)
        a, f, info = isim.ClosedLoop(C_, period_ns=p, uniform=uniform).arrivals(rec, k0 * C_, F_in)
        assert np.array_equal(a, want_a), (p, np.argwhere(a != want_a)[:4].tolist())
        assert np.array_equal(f, want_f)
        j = k0 * C_ + np.arange(n, dtype=np.int64)
        s = ((j % C_) * p // C_ if uniform else 0) + (j // C_) * p
        late = a.astype(np.int64) - s
        assert info.tolist() == [int(f.max()), int(f.min()), int((late > 0).sum()), int(late.sum())]


# ---- 3, 4. chaining and capture on the device
class DeviceBatch:
    def __init__(self, rec, C_, fill=0xA5):
        import torch
        self.torch, self.n, self.C = torch, len(rec), C_
        dev = torch.device("cuda", 0)
        self.rec = torch.from_numpy(rec.view(np.int64).copy()).to(dev)
        self.arr = torch.full((self.n,), -1, dtype=torch.int64, device=dev)
        self.free = torch.zeros(C_, dtype=torch.int64, device=dev)
        self.info = torch.full((4,), -1, dtype=torch.int64, device=dev)
        self.wsb = isim.closed_loop_workspace_bytes(self.n, C_)
        self.ws = torch.full((self.wsb,), fill, dtype=torch.uint8, device=dev)      # a dirty workspace

    def call(self, cl, lo, hi, first):
        """records [lo, hi) as one batch that starts at request first + lo, on the current stream"""
        cl.arrivals_device(self.rec.data_ptr() + 16 * lo, hi - lo, first + lo, d_free_at=self.free.data_ptr(),
                           d_arrivals=self.arr.data_ptr() + 8 * lo, d_info=self.info.data_ptr(),
                           d_workspace=self.ws.data_ptr(), workspace_bytes=self.wsb,
                           stream=self.torch.cuda.current_stream().cuda_stream)

    def host(self):
        self.torch.cuda.synchronize()
        return (self.arr.cpu().numpy().view(U64), self.free.cpu().numpy().view(U64),
                self.info.cpu().numpy().view(U64))


@pytest.mark.parametrize("C_", [3, 64, 1000])
def test_chaining_on_the_device(gpu, C_):
    n, first = 3 * 8192 + 5, 11
    rec = records(latencies("random", n, 5))
    cl = isim.ClosedLoop(C_, period_ns=400_000, uniform=True)
    want_a, want_f, want_i = cl.arrivals_host(rec, first)
    b = DeviceBatch(rec, C_)
    cuts = (0, 8192 + 1, 8192 + 1 + C_ // 2 + 1, n)
    for lo, hi in zip(cuts, cuts[1:]):
        b.call(cl, lo, hi, first)      # one stream, one workspace, no synchronisation in between
    a, f, info = b.host()
    assert np.array_equal(a, want_a) and np.array_equal(f, want_f)
    assert info[:2].tolist() == want_i[:2].tolist()      # the late totals are the last batch's alone


def test_dirty_workspace_and_capture(gpu):
    """The call captured in a graph with nothing run before it, replayed three times with the workspace, the
    outputs and the state refilled in between: the host function's values each time."""
    import torch
    n, first = 3 * 8192 + 5, 9
    for C_ in (4, 100):
        rec = records(latencies("random", n, 6))
        cl = isim.ClosedLoop(C_, period_ns=300_000)
        state = np.random.default_rng(C_).integers(0, 1 << 22, C_, dtype=np.uint64)
        want_a, want_f, want_i = cl.arrivals_host(rec, first, state)
        b = DeviceBatch(rec, C_, fill=0x5A)
        d_state = torch.from_numpy(state.view(np.int64).copy()).to(b.free.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            b.call(cl, 0, n, first)
        for fill in (0xC3, 0x00, 0xFF):
            b.ws.fill_(fill)
            b.arr.fill_(-1)
            b.info.fill_(-1)
            b.free.copy_(d_state)
            g.replay()
            a, f, info = b.host()
            assert np.array_equal(a, want_a) and np.array_equal(f, want_f) and np.array_equal(info, want_i), (C_, fill)


# ---- 5. end to end on a served walk
def test_timeline_of_a_served_walk(gpu):
    """64 connections at qps "max" over 20,000 served traces: every connection is busy until its last response,
    so exactly 64 requests are in flight at the end of every window up to ISIM_CL_MIN_FREE, and never more."""
    h = isim.Handler(isim.ServiceGraph.from_json(obj_to_json(config3p_topology(50, n=200))), None, isim.SimParams())
    n, C_ = 20_000, 64
    rec, _ = h.serve(0, n)
    a, f, info = isim.ClosedLoop(C_).arrivals(rec)
    assert np.array_equal(a, isim.ClosedLoop(C_).arrivals_host(rec)[0])
    makespan, min_free = int(info[native.CL_MAKESPAN]), int(info[native.CL_MIN_FREE])
    assert 0 < min_free <= makespan
    n_windows = 50
    window = makespan // (n_windows - 1) + 1      # the last window holds the makespan
    tl = isim.timeline(a, rec, window, n_windows)
    assert int(tl["arrived"].sum()) == n and int(tl["after"]["arrived"]) == 0
    ends = (np.arange(n_windows) + 1) * window
    in_flight = tl["in_flight_end"].astype(np.int64)
    assert (in_flight <= C_).all() and in_flight[-1] == 0
    full = ends <= min_free
    assert full.sum() > n_windows // 2 and (in_flight[full] == C_).all()


# ---- 6. ClosedLoopRun
def test_closed_loop_run_against_host_replay(gpu):
    doc = {"services": [
        {"name": "e", "isEntrypoint": True,
         "script": [{"sleep": "2ms"}, {"call": {"service": "a", "probability": 50}}]},
        {"name": "a", "script": [{"sleep": "3ms"}], "errorRate": 0.2}]}
    h = isim.Handler(isim.ServiceGraph.from_json(json.dumps(doc)), None, isim.SimParams())
    duration, window, batch = 10**9, 10**8, 512
    for cl in (isim.ClosedLoop(4), isim.ClosedLoop(4, qps=800, uniform=True)):
        r = isim.ClosedLoopRun(h, cl, duration, window, batch=batch, sub_bits=5).run(trace_begin=100)
        served = r["served"]
        assert served % batch == 0 and served > batch
        rec, _ = h.serve(100, served)
        a, f, info = cl.arrivals_host(rec)
        # it stopped at the first batch after which every connection is free at or after the duration
        assert int(info[native.CL_MIN_FREE]) >= duration and r["info"]["min_free_ns"] == int(info[native.CL_MIN_FREE])
        assert int(cl.arrivals_host(rec[:served - batch])[2][native.CL_MIN_FREE]) < duration
        assert np.array_equal(r["free_at"], f) and r["info"]["makespan_ns"] == int(info[native.CL_MAKESPAN])
        assert r["late"] == int(info[native.CL_LATE]) and r["sum_late_ns"] == int(info[native.CL_SUM_LATE])
        # numpy binning of the replay
        c = a + rec["latency_ns"]
        n_windows = duration // window
        wa, wc = np.minimum(a // U64(window), U64(n_windows)), np.minimum(c // U64(window), U64(n_windows))
        arrived = np.bincount(wa.astype(np.int64), minlength=n_windows + 1)
        code = (rec["status_err"] >> 31).astype(np.int64)
        tl = r["timeline"]
        assert tl["arrived"].tolist() == arrived[:n_windows].tolist()
        assert int(tl["after"]["arrived"]) == arrived[n_windows] == int((a >= U64(duration)).sum())
        for k in (0, 1):
            done = np.bincount(wc[code == k].astype(np.int64), minlength=n_windows + 1)
            assert tl["done"][k].tolist() == done[:n_windows].tolist() and int(tl["after"]["done"][k]) == done[n_windows]
            lat_sum = np.bincount(wc[code == k].astype(np.int64), weights=rec["latency_ns"][code == k].astype(np.float64),
                                  minlength=n_windows + 1)      # sums below 2^53: exact in doubles
            assert tl["sum_latency_ns"][k].tolist() == lat_sum[:n_windows].astype(np.int64).tolist()
        assert r["requests"] == int((a < U64(duration)).sum()) and r["achieved_qps"] == r["requests"] * 1e9 / duration
        # the sketch rows hold the same completions
        sk = r["sketch"]
        assert sk["count"][native.Q_ALL].tolist() == np.bincount(wc.astype(np.int64),
                                                                 minlength=n_windows + 1)[:n_windows].tolist()
        assert np.array_equal(r["sketch_table"],
                              isim.timeline_sketch_table(a, rec, window, n_windows, sub_bits=5))
    # the paced client is slower than the open one, and is late where a response outlasts its slot
    assert r["requests"] <= 800 and r["late"] > 0
