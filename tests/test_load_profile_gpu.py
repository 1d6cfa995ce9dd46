"""Load profiles on the GPU: isim_profile_arrivals* against a
numpy restatement of the rule (Philox, the Q24 exponential, a prefix sum, the
map by searchsorted), paced arrivals in closed form, the bound against the
constant-mean path, and both DES engines under a profile against level
restatements fed the exported arrivals."""
import json
import os

import numpy as np
import pytest

import isim
from isim import native
from isim.yamljson import yaml_to_json
from oracle import des_levels as dl
from oracle import graph_ref as gr
from oracle.executor_py import SimGraph

from conftest import TOPOLOGIES
from parity import oracle_params

pytestmark = pytest.mark.gpu

U64 = np.uint64
M32 = U64(0xFFFFFFFF)
Q = 1 << 24
CHUNK = 8192      # traces per arrivals chunk (csrc/load_profile.hip kChunk)
SEED = 0x5EED0123456789AB


# ---- the restatement
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


def trace_work_np(seed, begin, idx):
    """E(draw) of traces begin + idx (word 0 of philox((t_lo, t_hi, 0, 0x80000001)))."""
    t = np.asarray(idx, U64) + U64(begin)
    return exp_q24_np(dl.philox_np(t & M32, t >> U64(32), np.zeros(len(t), U64), np.full(len(t), 0x80000001, U64),
                                   seed)[0])


def work_np(seed, paced, begin, n):
    if paced:
        return (np.arange(n, dtype=U64) + U64(1)) << U64(24)
    return np.cumsum(trace_work_np(seed, begin, np.arange(n)), dtype=U64)    # below 2^61


def compile_np(segs):
    T = C = 0
    rows = []
    for j, (D, m) in enumerate(segs):
        rows.append((T, C, m))
        if j + 1 < len(segs):
            C = min(C + ((D << 24) // m if m else 0), 1 << 63)
            T += D
    return [np.array(x, dtype=object) for x in zip(*rows)]


def map_np(segs, u):
    """t(u) over a u64 array, in Python integers (object arrays): any product fits."""
    T, C, m = compile_np(segs)
    j = np.searchsorted(C.astype(U64), u, side="right") - 1       # the largest j with C_j <= u
    uo = u.astype(object)
    return (T[j] + (((uo - C[j]) * m[j]) >> 24)).astype(U64)


def arrivals_np(profile, seed, begin, n):
    return map_np(profile.segments, work_np(seed, profile.paced, begin, n))


def _doc(sleep="1ms"):
    return {"services": [{"name": "a", "isEntrypoint": True, "script": [{"sleep": sleep}]}]}


@pytest.fixture(scope="module")
def handler():
    return isim.Handler(isim.ServiceGraph.from_json(json.dumps(_doc())), None, isim.SimParams(seed=SEED))


def _ms_segments():
    """1024 segments of one millisecond at 20-60 us between arrivals, every 97th a pause."""
    segs = [(1_000_000, 0 if j % 97 == 96 else 20_000 + (j * 7919) % 40_000) for j in range(1023)]
    return segs + [(0, 30_000)]


PROFILES = {
    "one": [(0, 1000)],
    "light-heavy-light": [(5_000_000, 1000), (1_000_000, 100), (0, 1000)],
    "pause": [(3_000_000, 1000), (3_000_000_000, 0), (0, 700)],
    "1024ms": _ms_segments(),
}
SIZES = [1, 63, 8191, 8192, 8193, 3 * 8192 + 5]


def test_restatement_pieces():
    """The restatement's own parts against the oracle's scalar ones, and the map against the host function."""
    from oracle import des as od
    from oracle import philox as op
    us = np.array([0, 1, 255, 256, 0xFFFFFFFF, 0x80000000, 12345678], np.int64)
    assert exp_q24_np(us).tolist() == [od.exp_q24_py(int(u)) for u in us]
    t = (1 << 32) + 7
    want = od.exp_q24_py(op.philox4x32_10([t & 0xFFFFFFFF, t >> 32, 0, 0x80000001], (SEED & 0xFFFFFFFF, SEED >> 32))[0])
    assert int(trace_work_np(SEED, t, [0])[0]) == want
    for name, segs in PROFILES.items():
        p = isim.LoadProfile(segs)
        u = np.array([0, 1, Q, 5000 * Q, 5000 * Q + 1, 123456789 * Q + 99], U64)
        assert map_np(segs, u).tolist() == [p.time(int(x)) for x in u], name


@pytest.mark.parametrize("paced", [False, True])
@pytest.mark.parametrize("name", list(PROFILES))
def test_arrivals_against_restatement(gpu, handler, name, paced):
    p = isim.LoadProfile(PROFILES[name], paced=paced)
    for begin in (0, (1 << 32) - 100):
        want = arrivals_np(p, SEED, begin, SIZES[-1])     # a prefix of the largest case is every smaller one
        for n in SIZES:
            got = isim.profile_arrivals(handler, p, begin, n)
            assert got.dtype == np.uint64 and np.array_equal(got, want[:n]), \
                (begin, n, np.argwhere(got != want[:n])[:4].tolist())
    if name != "one":     # the cases do cross segments
        assert want[-1] > p.segments[0][0] + p.segments[1][0]
    assert isim.profile_arrivals(handler, p, 5, 0).size == 0


def test_paced_one_segment_is_exact(gpu, handler):
    for m in (1, 12345, 6_000_000, 1 << 34):
        got = isim.profile_arrivals(handler, isim.LoadProfile.constant(m, paced=True), 77, 20_000)
        assert np.array_equal(got, (np.arange(20_000, dtype=U64) + U64(1)) * U64(m)), m


def test_bound_against_constant_path(gpu, handler):
    """Sums of floors against the floor of the sum: 0 <= A_profile - A_const <= i + 1."""
    n = 3 * CHUNK + 5
    for m in (1, 999, 6_000_000, 1 << 34):
        a_const = isim.des_arrivals(handler, m, 4242, n).astype(object)
        a_prof = isim.profile_arrivals(handler, isim.LoadProfile.constant(m), 4242, n).astype(object)
        d = a_prof - a_const
        assert (d >= 0).all() and (d <= np.arange(1, n + 1)).all(), m
        # a mean that is a multiple of 2^24 floors nothing; any other does, and the two paths differ
        assert (d > 0).any() == (m % Q != 0), m


def test_past_one_scan_block_poisson(gpu, handler):
    """More than 1024 chunks: the scan of the chunk sums takes a second tier.  One segment of mean 2^24 ns makes
    t(u) = u, so arrivals are the work prefix itself and differences are exact: every chunk edge against the
    restated work of that trace, sampled runs against the small path (pinned above)."""
    n, begin = (1 << 23) + CHUNK + 3, 12345
    p = isim.LoadProfile.constant(Q)
    big = isim.profile_arrivals(handler, p, begin, n)
    assert np.array_equal(big[:70_001], work_np(SEED, False, begin, 70_001))
    assert (np.diff(big.astype(np.int64)) >= 0).all()
    edges = np.arange(CHUNK, n, CHUNK)
    assert np.array_equal(big[edges] - big[edges - 1], trace_work_np(SEED, begin, edges))
    rng = np.random.default_rng(3)
    ks = sorted(set(rng.integers(1, n - 64, 12).tolist() + [CHUNK * 1023 - 1, CHUNK * 1024 - 32, CHUNK * 1024, n - 64]))
    for k in ks:
        small = isim.profile_arrivals(handler, p, begin + k, 64)
        assert np.array_equal(big[k:k + 64] - big[k - 1], small), k


def test_past_one_scan_block_paced_segments(gpu, handler):
    """The map kernel over more than 1024 chunks and every segment of a 1024-segment profile, paced (work in
    closed form), against the restatement in u64: (u - C_j) m_j < 2^47 2^16."""
    n = (1 << 23) + CHUNK + 3
    segs = [(7_000_000, 0 if j % 97 == 96 else 500 + (j * 7919) % 1000) for j in range(1023)] + [(0, 777)]
    got = isim.profile_arrivals(handler, isim.LoadProfile(segs, paced=True), 0, n)
    T, C, m = (x.astype(U64) for x in compile_np(segs))
    u = work_np(SEED, True, 0, n)
    j = np.searchsorted(C, u, side="right") - 1
    want = T[j] + (((u - C[j]) * m[j]) >> U64(24))
    assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
    assert j[-1] == 1023 and len(np.unique(j)) > 1000


def test_dirty_workspace_and_capture(gpu, handler):
    """A 0xA5-filled workspace; then the call captured in a graph with nothing run before, replayed three
    times with the workspace refilled in between: the direct call's values each time."""
    import torch
    n, begin = 20_000, 99
    dev = torch.device("cuda", 0)
    wsb = isim.profile_arrivals_workspace_bytes(n)
    for name, paced in (("light-heavy-light", False), ("1024ms", False), ("pause", True)):
        p = isim.LoadProfile(PROFILES[name], paced=paced)
        want = arrivals_np(p, SEED, begin, n)
        ws = torch.full((wsb,), 0xA5, dtype=torch.uint8, device=dev)
        d_arr = torch.full((n,), -1, dtype=torch.int64, device=dev)
        s = torch.cuda.current_stream().cuda_stream
        isim.profile_arrivals_device(handler, p, begin, n, d_arrivals=d_arr.data_ptr(), d_workspace=ws.data_ptr(),
                                     workspace_bytes=wsb, stream=s)
        torch.cuda.synchronize()
        assert np.array_equal(d_arr.cpu().numpy().view(U64), want), name
        if name != "1024ms":
            continue
        ws2 = torch.full((wsb,), 0x5A, dtype=torch.uint8, device=dev)
        d2 = torch.full((n,), -1, dtype=torch.int64, device=dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            s = torch.cuda.current_stream().cuda_stream
            isim.profile_arrivals_device(handler, p, begin, n, d_arrivals=d2.data_ptr(), d_workspace=ws2.data_ptr(),
                                         workspace_bytes=wsb, stream=s)
        del p       # the graph holds the table's values, not the host profile
        for _ in range(3):
            ws2.fill_(0xC3)
            d2.fill_(-1)
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(d2.cpu().numpy().view(U64), want)


# ---- the engines under a profile
def levels_run(sg, op, begin, A):
    """oracle.des_levels.run with the arrivals given: (latency[n], wait_sum and wait_max per position,
    positions).  A replica's queue is FIFO in arrival order, ties in trace order (a stable sort), so callees
    of a replicated service, whose arrivals are not in trace order, are restated as well."""
    n = len(A)
    pos, depth = dl.unroll(sg, op, sg.entry())
    t = np.arange(begin, begin + n, dtype=U64)
    lo, hi = t & M32, t >> U64(32)
    A = A.astype(np.int64)
    S = np.zeros((len(pos), n), np.int64)
    wsum, wmax = np.zeros(len(pos), np.int64), np.zeros(len(pos), np.int64)
    for lvl in range(max(depth) + 1):
        for i in [k for k in range(len(pos)) if depth[k] == lvl]:
            q = pos[i]
            a = A if q["parent"] < 0 else S[q["parent"]] + q["off"]
            r = (dl.philox_np(lo, hi, np.full(n, i, U64), np.full(n, 0x80000002, U64), op.seed)[0] % U64(q["reps"])
                 if q["reps"] > 1 else np.zeros(n, U64))
            for rep in range(q["reps"]):
                ids = np.flatnonzero(r == U64(rep))
                ids = ids[np.argsort(a[ids], kind="stable")]
                if len(ids):
                    S[i, ids] = dl.fifo_starts(a[ids], q["hold"])
            w = S[i] - a
            wsum[i], wmax[i] = int(w.sum()), int(w.max())
    F = np.zeros_like(S)
    for i in reversed(range(len(pos))):
        q = pos[i]
        top = S[i] + q["floor"]
        if not q["leaf"]:
            for c in q["children"]:
                top = np.maximum(top, F[c])
            top = top + q["post"]
        F[i] = top
    return (F[0] - A).astype(U64), wsum, wmax, pos


class Case:
    def __init__(self, doc, profile, **kw):
        self.json = json.dumps(doc)
        self.h = isim.Handler(isim.ServiceGraph.from_json(self.json), None, isim.SimParams(**kw))
        self.d = isim.DesHandler(self.h, profile=profile)
        self.sg = SimGraph(gr.unmarshal_service_graph(self.json))
        self.op = oracle_params(self.h.params)

    def device(self, begin, n, wide):
        """One isim_serve_des_profile_device call into zeroed buffers: (records, stats, folded table)."""
        import torch
        dev = torch.device("cuda", 0)
        rec = torch.zeros(n * 2, dtype=torch.int64, device=dev)
        st = torch.zeros(self.h.stats_words, dtype=torch.int64, device=dev)
        tab = torch.zeros(max(1, self.d.table_words), dtype=torch.int64, device=dev)
        wsb = self.d.workspace_bytes(n)
        ws = torch.full((wsb // 8 + 1,), -1, dtype=torch.int64, device=dev)      # a dirty workspace
        self.d.serve_device(begin, n, rec.data_ptr(), st.data_ptr(), tab.data_ptr(), ws.data_ptr(), wsb,
                            torch.cuda.current_stream().cuda_stream, wide=wide)
        torch.cuda.synchronize()
        recs = rec.cpu().numpy().view(isim.REC_DTYPE)
        return recs, st.cpu().numpy().view(U64), self.d.fold(tab.cpu().numpy().view(U64))

    def check_table(self, rows, wsum, wmax, pos):
        for s in range(len(self.sg.g.services)):
            mine = [i for i, q in enumerate(pos) if q["svc"] == s]
            assert int(rows[s, native.DES_SUM_WAIT]) == sum(int(wsum[i]) for i in mine), s
            assert int(rows[s, native.DES_MAX_WAIT]) == max([int(wmax[i]) for i in mine] or [0]), s


def _tree13():
    doc = json.loads(yaml_to_json(open(os.path.join(TOPOLOGIES, "tree-13-services.yaml"), "rb").read()))
    doc["defaults"]["numReplicas"] = 1
    for s in doc["services"]:
        s["script"] = [{"sleep": "400us" if s["name"] == "d" else "150us"}] + s.get("script", [])
        if s["name"] == "svc-0-1":
            s["numReplicas"] = 3
    return doc


@pytest.mark.parametrize("wide", [False, True])
def test_static_engine_under_profile(gpu, wide):
    """tree-13 with sleeps, 3 replicas on one inner service; light (no queueing) / overload (gaps of 100 us
    against the entry's 400 us hold) / light."""
    n, begin = 20_000, 1000
    light, over = 2_000_000, 100_000
    p = isim.LoadProfile.steps([(5000 * light, light), (3000 * over, over)], light)
    c = Case(_tree13(), p)
    assert c.d.info.items == 0
    A = c.d.arrivals(begin, n)
    assert np.array_equal(A, arrivals_np(p, c.h.params.seed, begin, n))
    lat, wsum, wmax, pos = levels_run(c.sg, c.op, begin, A)
    recs, stats, rows = c.device(begin, n, wide)
    assert stats[native.ST_DES_RETRY] == 0 and stats[native.ST_N_TRACES] == n
    assert np.array_equal(recs["latency_ns"], lat), np.argwhere(recs["latency_ns"] != lat)[:4].tolist()
    c.check_table(rows, wsum, wmax, pos)
    # the synchronous call: the same numbers
    srecs, sstats, stab = c.d.serve(begin, n)
    assert np.array_equal(srecs["latency_ns"], lat) and np.array_equal(c.d.fold(stab), rows)
    # the overload shows: latencies of arrivals inside the overload segment pass anything the first light one saw
    t1, t2 = 5000 * light, 5000 * light + 3000 * over
    first, mid = A < U64(t1), (A >= U64(t1)) & (A < U64(t2))
    assert first.sum() > 1000 and mid.sum() > 1000
    assert lat[mid].max() > lat[first].max()
    assert lat[mid].max() > 50 * 400_000      # a queue of tens of holds at the entry


def test_pause_of_three_seconds(gpu):
    """Two bursts 3 s apart: the pause lies inside one 64-trace group, whose 32-bit rows cannot hold A_t - G
    (3e9 > 2^31).  The device call either accumulates the restatement's numbers or counts the batch in
    ISIM_ST_DES_RETRY and accumulates nothing; the synchronous call returns the restatement's latencies."""
    n, begin = 2000, 0
    p = isim.LoadProfile([(990 * 300_000 + 1, 300_000), (3_000_000_000, 0), (0, 300_000)], paced=True)
    c = Case(_tree13(), p)
    A = c.d.arrivals(begin, n)
    gaps = np.diff(A.astype(np.int64))
    k = int(np.argmax(gaps))
    assert gaps[k] >= 3_000_000_000 and (k + 1) % 64 != 0      # inside a group
    lat, wsum, wmax, pos = levels_run(c.sg, c.op, begin, A)
    recs, stats, rows = c.device(begin, n, wide=False)
    if stats[native.ST_DES_RETRY]:
        assert stats[native.ST_DES_RETRY] == 1 and stats[native.ST_N_TRACES] == 0 and rows.sum() == 0
    else:
        assert np.array_equal(recs["latency_ns"], lat)
    recs, stats, rows = c.device(begin, n, wide=True)
    assert stats[native.ST_DES_RETRY] == 0 and np.array_equal(recs["latency_ns"], lat)
    c.check_table(rows, wsum, wmax, pos)
    srecs, sstats, stab = c.d.serve(begin, n)
    assert sstats[native.ST_DES_RETRY] == 0 and np.array_equal(srecs["latency_ns"], lat)
    c.check_table(c.d.fold(stab), wsum, wmax, pos)


def test_item_engine_under_profile(gpu):
    """Probability-50 calls, only the entry sleeps (one replica): the entry's queue is the only one, so
    latency_t = (S_t - A_t) + T_walk(t), S the FIFO starts over the exported arrivals and T_walk the plain
    walk's latency of the same trace."""
    P, n, begin = 500_000, 20_000, 31
    doc = {"services": [
        {"name": "e", "isEntrypoint": True,
         "script": [{"sleep": "500us"}, [{"call": {"service": "a", "probability": 50}},
                                         {"call": {"service": "b", "probability": 50}}]]},
        {"name": "a", "script": [{"call": {"service": "c", "probability": 50}}]},
        {"name": "b"}, {"name": "c"}]}
    p = isim.LoadProfile.steps([(4000 * 2_000_000, 2_000_000), (6000 * 250_000, 250_000)], 1_000_000)
    c = Case(doc, p)
    assert c.d.info.items == 1
    A = c.d.arrivals(begin, n)
    assert np.array_equal(A, arrivals_np(p, c.h.params.seed, begin, n))
    walk, _ = c.h.serve(begin, n, device=0)
    S = dl.fifo_starts(A, P)
    want = (S - A.astype(np.int64)).astype(U64) + walk["latency_ns"]
    recs, stats, table = c.d.serve(begin, n)
    assert np.array_equal(recs["latency_ns"], want), np.argwhere(recs["latency_ns"] != want)[:4].tolist()
    assert np.array_equal(recs["hops"], walk["hops"])
    assert ((S - A.astype(np.int64)) > 0).sum() > 3000      # the second step does queue
    drecs, dstats, rows = c.device(begin, n, wide=False)
    assert np.array_equal(drecs["latency_ns"], want) and dstats[native.ST_DES_RETRY] == 0


@pytest.mark.parametrize("begin", [0, 1_000_003])
@pytest.mark.parametrize("paced", [False, True])
def test_profile_arrivals_are_the_engines(gpu, begin, paced):
    """One service, one replica, one sleep P: the Lindley recursion over isim.profile_arrivals,
    S_t = max(A_t, S_{t-1} + P), gives isim_serve_des_profile's latency S_t + P - A_t for every trace."""
    P, n = 1_000_000, 20_000
    p = isim.LoadProfile.steps([(3 * 10**9, 3_000_000), (2 * 10**9, 800_000), (10**9, 0)], 1_500_000, paced=paced)
    h = isim.Handler(isim.ServiceGraph.from_json(json.dumps(_doc("1ms"))), None, isim.SimParams())
    d = isim.DesHandler(h, profile=p)
    recs, _, _ = d.serve(begin, n, device=0)
    A = isim.profile_arrivals(h, p, begin, n).astype(np.int64)
    t = np.arange(n, dtype=np.int64)
    S = t * P + np.maximum.accumulate(A - t * P)
    want = (S + P - A).astype(U64)
    assert np.array_equal(recs["latency_ns"], want), np.argwhere(recs["latency_ns"] != want)[:4].tolist()
    assert (want > P).sum() > n // 20      # the queue forms in the heavy step


def test_paced_timeline_counts(gpu):
    """Paced steps: the arrivals per window of DesHandler(profile=...).timeline are the counts of the rule
    in Python integers."""
    segs = [(10**9, 1_000_000), (10**9, 250_000), (2 * 10**9, 0), (0, 500_000)]
    p = isim.LoadProfile(segs, paced=True)
    h = isim.Handler(isim.ServiceGraph.from_json(json.dumps(_doc("100us"))), None, isim.SimParams())
    n, window, n_windows = 9000, 250_000_000, 24
    tl = isim.DesHandler(h, profile=p).timeline(0, n, window, n_windows)
    counts = [0] * (n_windows + 1)
    for i in range(n):
        counts[min(p.time((i + 1) << 24) // window, n_windows)] += 1
    assert tl["arrived"].tolist() == counts[:n_windows] and int(tl["after"]["arrived"]) == counts[n_windows]
    # arrival i comes at (i + 1) ms: 999 before 1 s, the 1000th at 1 s sharp and 3999 more at 4 per ms, none
    # in the pause, then 2 per ms from 4 s; the last at 6 s sharp, past the last window
    assert sum(counts[:4]) == 999 and sum(counts[4:8]) == 4000 and sum(counts[8:16]) == 0
    assert counts[16:24] == [500] * 8 and counts[24] == 1
