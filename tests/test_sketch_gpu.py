"""The mergeable latency sketch on the GPU: isim_latency_sketch*
and isim_timeline_sketch* word for word against np.bincount over the bucket rule
restated here (rows in Python integers), the bracket property against the exact
selects (§13, §15), accumulation against the host merge, guard words and graph
capture, and DesHandler.timeline_sketch on an overloaded tree.  Every
comparison is equality of integers or a bracket condition."""
import json
import os

import numpy as np
import pytest

import isim
from isim import native
from isim.yamljson import yaml_to_json

from conftest import TOPOLOGIES
from test_timeline_gpu import WINDOWS, make_case, make_recs, rows_of

pytestmark = pytest.mark.gpu

U64 = np.uint64
MAXU = (1 << 64) - 1
BIT31 = np.uint32(1 << 31)
STEP = 2048      # records a workgroup takes per step (csrc/sketch.hip kStep)
TILE = 4 * STEP  # records per workgroup of the per-window kernel (kTile)
NAMES = ("all", "200", "500")


# ---- the rule restated over u64 arrays (shifts and compares only), pinned to Python integers
def bins_of(s):
    return (65 - s) * 2**s


def bitlen_np(v):
    x = np.asarray(v, U64).copy()
    n = np.zeros(x.shape, np.int64)
    for sh in (32, 16, 8, 4, 2, 1):
        m = x >= (U64(1) << U64(sh))
        n += m * sh
        x = np.where(m, x >> U64(sh), x)
    return n + (x > 0)


def bucket_np(s, v):
    v = np.asarray(v, U64)
    shift = np.maximum(bitlen_np(v) - (s + 1), 0)
    b = (shift << s) + (v >> shift.astype(U64)).astype(np.int64)
    chk = [int(x) for x in v[:: max(1, len(v) // 64)]]
    for x, got in zip(chk, b[:: max(1, len(v) // 64)]):
        sh = max(0, x.bit_length() - (s + 1))
        assert int(got) == sh * 2**s + x // 2**sh
    return b


def py_bounds(s, b):
    if b < 2 ** (s + 1):
        return b, b
    shift = b // 2**s - 1
    lo = (2**s + b % 2**s) * 2**shift
    return lo, lo + 2**shift - 1


def codes(recs):
    return ((recs["status_err"] & BIT31) != 0).astype(np.int64)


def expect_table(recs, s):
    key = codes(recs) * bins_of(s) + bucket_np(s, recs["latency_ns"])
    return np.bincount(key, minlength=2 * bins_of(s)).astype(U64)


def expect_windowed(arr, recs, t0, window, n_windows, s):
    arr = np.asarray(arr, U64)
    lat = recs["latency_ns"].astype(U64)
    c = arr + lat
    c = np.where(c < arr, U64(MAXU), c)  # saturates
    rc = rows_of(c, t0, window, n_windows) if len(arr) else np.zeros(0, np.int64)
    key = (rc * 2 + codes(recs)) * bins_of(s) + bucket_np(s, lat)
    return np.bincount(key, minlength=(n_windows + 2) * 2 * bins_of(s)).astype(U64)


def differ(got, want, s):
    bad = np.argwhere(got != want)[:4, 0]
    w = 2 * bins_of(s)
    return [(int(i) // w, int(i) % w // bins_of(s), int(i) % bins_of(s), int(got[i]), int(want[i])) for i in bad]


def check(recs, s, note=None):
    got = isim.latency_sketch(recs, s)
    want = expect_table(recs, s)
    assert got.dtype == np.uint64 and np.array_equal(got, want), (note, s, differ(got, want, s))
    assert int(got.sum()) == len(recs)
    return got


def octave_latencies(n, seed):
    """Bit lengths uniform in 0..64: every octave is hit."""
    rng = np.random.default_rng(seed)
    bl = rng.integers(0, 65, n)
    v = rng.integers(0, 1 << 64, n, dtype=np.uint64) | U64(1 << 63)
    v = np.where(bl == 0, U64(0), v >> (U64(64) - np.maximum(bl, 1).astype(U64)))
    forced = np.array([MAXU, 0, 1 << 63, 255, 256, 257], U64)[:n]
    v[rng.permutation(n)[:len(forced)]] = forced
    return v


@pytest.mark.parametrize("s", [0, 3, 7])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, STEP - 1, STEP, STEP + 1, (1 << 20) + 3])
def test_whole_batch_every_octave(gpu, n, s):
    recs = make_recs(octave_latencies(n, n + s), n)
    t = check(recs, s)
    if n >= 6:
        assert t.reshape(2, -1)[:, 0].sum() >= 1 and t.reshape(2, -1)[:, -1].sum() >= 1   # 0 and 2^64 - 1


@pytest.mark.parametrize("s", [0, 3, 7])
def test_all_lanes_one_word(gpu, s):
    """A constant batch (a static walk without draws): 64 lanes on one word, also 0 and 2^64 - 1;
    then every record a 200, every record a 500."""
    for value in (8_000_000, 0, MAXU):
        for n in (64, 320, 5000):
            recs = make_recs(np.full(n, value, U64), n)
            recs["status_err"] &= ~BIT31
            t = check(recs, s, value).reshape(2, -1)
            b = int(bucket_np(s, np.array([value], U64))[0])
            assert t[0, b] == n
            recs["status_err"] |= BIT31
            assert check(recs, s, value).reshape(2, -1)[1, b] == n
    recs = make_recs(octave_latencies(5000, 3), 4)
    recs["status_err"] &= ~BIT31
    assert not check(recs, s).reshape(2, -1)[1].any()
    recs["status_err"] |= BIT31
    assert not check(recs, s).reshape(2, -1)[0].any()


@pytest.mark.parametrize("s", [0, 3, 7])
def test_all_lanes_different_bins_and_bin_edges(gpu, s):
    """Each wave's 64 lanes on 64 different bins; then lo - 1, lo and lo + 1 of every bin."""
    bins = bins_of(s)
    los = np.array([py_bounds(s, b)[0] for b in range(bins)], U64)
    pick = los[np.arange(640) % 64 * (bins // 64)]
    assert len(set(bucket_np(s, pick[:64]).tolist())) == 64
    recs = make_recs(pick, 5)
    recs["status_err"] &= ~BIT31
    t = check(recs, s).reshape(2, -1)
    assert (t[0] == 10).sum() == 64
    edges = np.concatenate([los[1:] - U64(1), los, los[:-1] + U64(1), np.array([MAXU], U64)])
    t = check(make_recs(edges, 6), s).reshape(2, -1)
    assert (t.sum(axis=0) >= 2).all()   # its lo and the hi below the next lo, in every bin


def _upload(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(torch.device("cuda", 0))


class Guarded:
    """A zeroed device table with 0xA5-filled regions on both sides."""
    PAD = 4096

    def __init__(self, torch, words):
        self.torch, self.words = torch, words
        self.buf = torch.full((words * 8 + 2 * self.PAD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        self.buf[self.PAD:self.PAD + words * 8] = 0
        self.ptr = self.buf.data_ptr() + self.PAD

    def result(self):
        self.torch.cuda.synchronize()
        h = self.buf.cpu().numpy()
        assert (h[:self.PAD] == 0xA5).all() and (h[-self.PAD:] == 0xA5).all(), "a guard word was written"
        return h[self.PAD:-self.PAD].view(U64).copy()


@pytest.mark.parametrize("s", [0, 3, 7])
def test_offset_accumulation_guards_and_capture(gpu, s):
    """Records at a pointer offset by one record; two calls into one table = twice one call = the host
    merge; the table's neighbours stay 0xA5; a captured call replayed three times gives 3 x one call."""
    import torch
    n = 3 * STEP + 77
    recs = make_recs(octave_latencies(n + 1, 40 + s), 41)
    d_rec = _upload(torch, recs)
    stream = torch.cuda.current_stream().cuda_stream
    one = expect_table(recs[1:], s)
    g = Guarded(torch, isim.sketch_words(s))
    isim.latency_sketch_device(d_rec.data_ptr() + 16, n, s, d_table=g.ptr, stream=stream)
    assert np.array_equal(g.result(), one), differ(g.result(), one, s)
    isim.latency_sketch_device(d_rec.data_ptr() + 16, n, s, d_table=g.ptr, stream=stream)
    twice = g.result()
    assert np.array_equal(twice, one * U64(2))
    assert np.array_equal(twice, isim.sketch_merge(s, one.copy(), one))
    isim.latency_sketch_device(0, 0, s, d_table=g.ptr, stream=stream)   # no records: nothing touched
    assert np.array_equal(g.result(), twice)
    # the synchronous form accumulates as well
    assert np.array_equal(isim.latency_sketch(recs[1:], s, out=one.copy()), twice)
    # capture, with nothing of this table run before it
    c = Guarded(torch, isim.sketch_words(s))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        isim.latency_sketch_device(d_rec.data_ptr() + 16, n, s, d_table=c.ptr,
                                   stream=torch.cuda.current_stream().cuda_stream)
    for _ in range(3):
        graph.replay()
    assert np.array_equal(c.result(), one * U64(3))


# ---- the bracket property: a condition, not a tolerance
def _walk_batch(seed_begin, n):
    doc = {"services": [
        {"name": "a", "isEntrypoint": True, "errorRate": 0.1,
         "script": [{"call": {"service": "b", "probability": 50}}, {"call": {"service": "c", "probability": 30}}]},
        {"name": "b", "errorRate": 0.2, "script": [{"sleep": "1ms"}, {"call": {"service": "c", "probability": 70}}]},
        {"name": "c", "script": [{"sleep": "3ms"}]}]}
    h = isim.Handler(isim.ServiceGraph.from_json(json.dumps(doc)), None, isim.SimParams())
    assert h.info.static_walk == 0
    recs, _ = h.serve(seed_begin, n, device=0)
    return recs


def _des_batch(begin, n):
    from isim.generators import realistic_topology
    from isim.yamljson import obj_to_json
    j = obj_to_json(realistic_topology(120, concurrent=True, sleep_ms=(1, 5), error_rate=(0.0, 0.05)))
    h = isim.Handler(isim.ServiceGraph.from_json(j), None, isim.SimParams())
    recs, _, _ = isim.DesHandler(h, 6_000_000).serve(begin, n, device=0)
    return recs


@pytest.fixture(scope="module")
def served(gpu):
    """The batches of the bracket tests and their exact percentiles, computed once."""
    walk, walk2, des = _walk_batch(12345, 4096), _walk_batch(900_000, 3000), _des_batch(0, 3000)
    return {"walk": (walk, isim.latency_quantiles(walk)), "des": (des, isim.latency_quantiles(des)), "walk2": walk2}


def assert_brackets(s, table, exact, note):
    got = isim.sketch_quantiles(s, table)
    for name in NAMES:
        assert got[name]["count"] == exact[name]["count"], (note, name)
        for f in isim.DEFAULT_Q:
            lo, hi = got[name]["q"][f]
            assert lo <= exact[name]["q"][f] <= hi, (note, s, name, f, lo, exact[name]["q"][f], hi)
            assert hi - lo < max(1, lo >> s), (note, s, name, f, lo, hi)


@pytest.mark.parametrize("s", [0, 3, 7])
def test_brackets_contain_the_exact_percentiles(gpu, served, s):
    for kind in ("walk", "des"):
        recs, exact = served[kind]
        assert exact["all"]["count"] == len(recs) and exact["200"]["count"] > 0
        table = isim.latency_sketch(recs, s)
        assert np.array_equal(table, expect_table(recs, s))
        assert_brackets(s, table, exact, kind)
    # two batches sketched into one table, against numpy on their concatenation
    a, b = served["walk"][0], served["walk2"]
    table = isim.latency_sketch(b, s, out=isim.latency_sketch(a, s))
    both = np.concatenate([a, b])
    exact = {}
    is500 = codes(both).astype(bool)
    for name, mask in (("all", np.ones(len(both), bool)), ("200", ~is500), ("500", is500)):
        v = np.sort(both["latency_ns"][mask])
        exact[name] = {"count": len(v), "q": {f: int(v[max(1, -(-round(f * 1e6) * len(v) // 10**6)) - 1])
                                              for f in isim.DEFAULT_Q}}
    assert_brackets(s, table, exact, "two batches")


# ---- per window
def sub_bits_for(n_windows):
    """Every sub_bits where the table stays small; the 65,538-row table only at s = 0 (68 MB)."""
    return (0,) if n_windows > 4096 else (0, 3) if n_windows > 64 else (0, 3, 7)


def check_windowed(arr, recs, t0, window, n_windows, s, note=None):
    got = isim.timeline_sketch_table(arr, recs, window, n_windows, t0, s)
    want = expect_windowed(arr, recs, t0, window, n_windows, s)
    assert np.array_equal(got, want), (note, s, differ(got, want, s))
    return got.reshape(n_windows + 2, 2, bins_of(s))


@pytest.mark.parametrize("n", [0, 1, 65, TILE - 1, TILE + 1, 20_001])
@pytest.mark.parametrize("window,n_windows", WINDOWS)
def test_windowed_against_numpy(gpu, n, window, n_windows):
    """Sorted and permuted arrivals, completions that saturate (make_case), both t0 values."""
    for t0_mode in (0, 1):
        arr, recs, t0 = make_case(n, window, n_windows, t0_mode, seed=n * 7 + n_windows + t0_mode)
        for permuted in (False, True):
            if permuted:
                p = np.random.default_rng(n).permutation(n)
                arr, recs = arr[p], recs[p]
            for s in sub_bits_for(n_windows):
                t = check_windowed(arr, recs, t0, window, n_windows, s, (t0_mode, permuted))
                assert int(t.sum()) == n
                # the rows summed are the whole-batch table
                assert np.array_equal(t.sum(axis=0).reshape(-1), expect_table(recs, s))


@pytest.mark.parametrize("s", [0, 3, 7])
def test_windowed_constant_and_run_edges(gpu, s):
    """All lanes on one word of one row; then completions spread over more rows than the LDS run
    holds at any sub_bits (200 rows), ascending, so tiles anchor in the middle and at the last rows."""
    for n in (64, 5000):
        recs = make_recs(np.full(n, 8_000_000, U64), n)
        recs["status_err"] &= ~BIT31
        t = check_windowed(np.full(n, 123_456_789, U64), recs, 0, 10**6, 200, s)
        assert t[132, 0, int(bucket_np(s, np.array([8_000_000], U64))[0])] == n
    n = 3 * TILE + 5
    arr = (np.arange(n, dtype=U64) * U64(200 * 10**6)) // U64(n)
    recs = make_recs(np.random.default_rng(s).integers(0, 3 * 10**6, n, dtype=np.uint64), 8)
    t = check_windowed(arr, recs, 0, 10**6, 198, s)
    assert (t.sum(axis=(1, 2)) > 0).sum() >= 199


def test_windowed_against_the_timeline_and_the_exact_select(gpu):
    """Each row's per-code totals are isim_timeline's DONE words, and each row's brackets contain
    isim_timeline_quantiles' exact values."""
    for window, n_windows in ((7, 37), (10**6, 30)):
        arr, recs, t0 = make_case(9000, window, n_windows, 1, seed=n_windows)
        tl = isim.timeline_table(arr, recs, window, n_windows, t0).reshape(n_windows + 2, native.TL_ROW_WORDS)
        tq = isim.timeline_quantiles(arr, recs, window, n_windows, t0)
        for s in (0, 3, 7):
            d = isim.timeline_sketch(arr, recs, window, n_windows, t0, s)
            t = d["table"].reshape(n_windows + 2, 2, bins_of(s))
            for code in (0, 1):
                assert np.array_equal(t[:, code].sum(axis=1), tl[:, native.TL_DONE + code])
            assert d["q"] == tq["q"] == isim.DEFAULT_Q
            for part in (None, "before", "after"):
                sk, ex = (d, tq) if part is None else (d[part], tq[part])
                assert np.array_equal(sk["count"], ex["count"])
                lo, hi, v = sk["lo_ns"], sk["hi_ns"], ex["latency_ns"]
                assert (lo <= v).all() and (v <= hi).all(), (window, s, part)
                assert (hi - lo < np.maximum(U64(1), lo >> U64(s))).all()
            assert d["count"].sum() > 0 and d["after"]["count"].sum() > 0


@pytest.mark.parametrize("s", [3, 7])
def test_windowed_accumulation_guards_and_capture(gpu, s):
    """Two device calls into one table = the host merge of two single tables = one call over the
    concatenation; the table's neighbours stay 0xA5; capture and three replays give 3 x one call."""
    import torch
    window, n_windows = 10**6, 30
    a1, r1, _ = make_case(9000, window, n_windows, 0, seed=21)
    a2, r2, _ = make_case(4001, window, n_windows, 0, seed=22)
    t1 = isim.timeline_sketch_table(a1, r1, window, n_windows, 0, s)
    t2 = isim.timeline_sketch_table(a2, r2, window, n_windows, 0, s)
    both = expect_windowed(np.concatenate([a1, a2]), np.concatenate([r1, r2]), 0, window, n_windows, s)
    assert np.array_equal(isim.sketch_merge(s, t1.copy(), t2), both)
    assert np.array_equal(isim.timeline_sketch_table(a2, r2, window, n_windows, 0, s, out=t1.copy()), both)
    words = isim.timeline_sketch_out_words(n_windows, s)
    g = Guarded(torch, words)
    stream = torch.cuda.current_stream().cuda_stream
    bufs = [(_upload(torch, a), _upload(torch, r), len(a)) for a, r in ((a1, r1), (a2, r2))]
    for da, dr, n in bufs:
        isim.timeline_sketch_device(da.data_ptr(), dr.data_ptr(), n, window, n_windows, 0, s, d_out=g.ptr,
                                    stream=stream)
    assert np.array_equal(g.result(), both)
    isim.timeline_sketch_device(0, 0, 0, window, n_windows, 0, s, d_out=g.ptr, stream=stream)
    assert np.array_equal(g.result(), both)
    c = Guarded(torch, words)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        da, dr, n = bufs[0]
        isim.timeline_sketch_device(da.data_ptr(), dr.data_ptr(), n, window, n_windows, 0, s, d_out=c.ptr,
                                    stream=torch.cuda.current_stream().cuda_stream)
    for _ in range(3):
        graph.replay()
    assert np.array_equal(c.result(), t1 * U64(3))


def test_end_to_end_des(gpu):
    """DesHandler.timeline_sketch on the committed 13-service tree with a 2 ms sleep in every
    service, at a 1 ms mean gap (overloaded: the queue grows, and the p99 bracket with it)."""
    doc = json.loads(yaml_to_json(open(os.path.join(TOPOLOGIES, "tree-13-services.yaml"), "rb").read()))
    for svc in doc["services"]:
        svc["script"] = [{"sleep": "2ms"}] + (svc.get("script") or [])
        svc["errorRate"] = 0.05
    h = isim.Handler(isim.ServiceGraph.from_json(json.dumps(doc)), None, isim.SimParams())
    d = isim.DesHandler(h, 1_000_000)
    n, begin, window, n_windows, s = 6000, 17, 250_000_000, 20, 7
    sk = d.timeline_sketch(begin, n, window, n_windows)
    recs, _, _ = d.serve(begin, n)
    arr = d.arrivals(begin, n)
    assert np.array_equal(sk["table"], expect_windowed(arr, recs, 0, window, n_windows, s))
    exact = d.timeline_quantiles(begin, n, window, n_windows)
    assert sk["q"] == isim.DEFAULT_Q
    for part in (None, "after"):
        a, e = (sk, exact) if part is None else (sk[part], exact[part])
        assert np.array_equal(a["count"], e["count"])
        assert (a["lo_ns"] <= e["latency_ns"]).all() and (e["latency_ns"] <= a["hi_ns"]).all()
        assert (a["hi_ns"] - a["lo_ns"] < np.maximum(U64(1), a["lo_ns"] >> U64(s))).all()
    assert not sk["before"]["count"].any()
    assert int(sk["count"][native.Q_ALL].sum() + sk["after"]["count"][native.Q_ALL]) == n
    assert sk["count"][native.Q_500].sum() > 0
    p99 = sk["lo_ns"][native.Q_200, isim.DEFAULT_Q.index(0.99)]
    assert 0 < p99[1] <= p99[n_windows // 2] <= p99[-1]
