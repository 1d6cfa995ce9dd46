"""DES worker pools on the GPU: every field of the whole
batch's spans (isim_serve_des_spans_device, threshold 0), the records and the
folded DES table against the pooled event-driven restatement
(tests/des_workers_ref.py, checked on the CPU by tests/test_des_workers.py):
pools around k_qscan's tile sizes, replicas, rounds that mix pooled and
single-worker rows, every source of a round's order with both scans and both
sorts, ties, the unchanged default, the pool's bound on the device's spans
alone, and the service timeline and the DES critical path over a pooled batch."""
import functools

import numpy as np
import pytest

import isim
from isim import native

import des_workers_ref as ref
from test_des_gpu import DesCase
from test_des_spans_gpu import run_tap
from test_des_workers import BEGIN, GRAPHS, case, paced_arrivals, reference, worker_list

pytestmark = pytest.mark.gpu

SBK, TWO = native.FLAG_DES_SCAN_BY_KEY, native.FLAG_DES_TWO_SORTS
FIELDS = ("arrival_ns", "start_ns", "finish_ns", "hop_ns", "hop", "caller_hop", "position", "service", "status",
          "replica")


@functools.lru_cache(maxsize=None)
def _device(name, wl, flags, begin, n, paced):
    c = case(name, flags)
    d = c.d
    if paced:
        d = isim.DesHandler(c.h, profile=isim.LoadProfile.constant(GRAPHS[name][3], paced=True))
    d.workers = list(wl)
    assert d.workers.tolist() == list(wl)
    r = run_tap(c, begin, n, d=d)
    total = int(r["off"][n])
    assert list(r["info"]) == [total, n, n, n, n]
    assert int(r["stats"][native.ST_DES_RETRY]) == 0
    return c, r, r["spans"][:total]


def device(name, workers, flags=0, begin=BEGIN, n=None, paced=False):
    """The whole batch of graph `name` under `workers`, tapped: one device call shared by the tests."""
    c = case(name, flags)
    return _device(name, tuple(worker_list(c, workers)), flags, begin, GRAPHS[name][4] if n is None else n, paced)


def equals_the_restatement(c, r, s, want):
    assert len(s) == len(want)
    for f in FIELDS:
        bad = np.flatnonzero(s[f] != want[f])
        assert bad.size == 0, (f, bad[:4], s[bad[:4]], want[bad[:4]])
    recs = r["recs"]
    assert np.array_equal(recs["latency_ns"], ref.latencies(want))
    assert np.array_equal(recs["hops"], np.bincount((want["trace"] - want["trace"][0]).astype(np.int64)))
    assert np.array_equal(recs["status_err"] >> 31, want[want["hop"] == 0]["status"] & 1)
    rows = c.d.fold(r["table"])
    t = ref.table_of(want, c.h.info.n_services)
    assert np.array_equal(rows[:, native.DES_COUNT], t[:, 0])
    assert np.array_equal(rows[:, native.DES_SUM_WAIT], t[:, 1])
    assert np.array_equal(rows[:, native.DES_MAX_WAIT], t[:, 2])
    assert np.array_equal(rows[:, 2 * native.N_PROM] + rows[:, 2 * native.N_PROM + 1], t[:, 3])
    hold = np.array(ref.holds(c.sg), np.uint64)
    assert np.array_equal(rows[:, native.DES_SUM_HOLD], t[:, 0] * hold)
    # the wait table of the tap is the same batch's
    ns = c.h.info.n_services
    assert np.array_equal(r["wait"][:ns, native.DW_SUM_WAIT], t[:, 1])


def at_most_w_busy(c, s, wl):
    """On the device's spans alone: at no instant are more than W_s spans of one (service, replica) between
    their start and start + hold."""
    hold = ref.holds(c.sg)
    for svc in np.unique(s["service"]):
        P, W = hold[int(svc)], wl[int(svc)]
        if P == 0:
            continue
        m = s["service"] == svc
        for rep in np.unique(s["replica"][m]):
            S = np.sort(s["start_ns"][m & (s["replica"] == rep)])
            busy = np.arange(1, len(S) + 1) - np.searchsorted(S + np.uint64(P), S, side="right")
            assert int(busy.max()) <= W, (int(svc), int(rep), int(busy.max()), W)


def check(name, workers, flags=0, begin=BEGIN, n=None, paced=False):
    c, r, s = device(name, workers, flags, begin, n, paced)
    nn = GRAPHS[name][4] if n is None else n
    arr = paced_arrivals(GRAPHS[name][3], nn) if paced else None
    equals_the_restatement(c, r, s, reference(name, workers, begin, nn, arr))
    at_most_w_busy(c, s, worker_list(c, workers))
    return c, r, s


@pytest.mark.parametrize("W", [1, 2, 3, 63, 64, 65, 511, 513, 4096])
def test_pools_around_the_scan_tiles(gpu, W):
    """One replica's 3,000 requests: a segment over six 512-item k_qscan tiles, its classes cut anywhere."""
    c, r, s = check("two", W)
    b = s[s["service"] == 1]
    assert len(b) == 3000
    assert bool(np.any(b["start_ns"] > b["arrival_ns"])) == (W < 3000)


@pytest.mark.parametrize("W", [2, 5])
def test_replicas(gpu, W):
    c, r, s = check("two_reps", W)
    assert len(np.unique(s["replica"][s["service"] == 1])) == 3


def test_a_round_of_pooled_and_single_rows(gpu):
    c, r, s = check("mixed", GRAPHS["mixed"][5])
    w = s["start_ns"] > s["arrival_ns"]
    names = [x["name"] for x in c.h.graph.canonical()["services"]]
    assert np.any(w & (s["service"] == names.index("b"))) and np.any(w & (s["service"] == names.index("c")))
    assert not np.any(w & (s["service"] == names.index("z")))   # no hold: nobody ever waits for z


def test_a_sort_free_round_with_zero_holds_by_key(gpu):
    """b (3 workers) and the zero-hold z in one sort-free round under ISIM_FLAG_DES_SCAN_BY_KEY: the list written
    out by k_pairs<kQList>, z's items under keys that differ from both neighbours', read by wk_head and then by
    rocPRIM's scan by key; k_qscan over the same refined arrays agrees.  (zero_hold_mix itself cannot carry a
    pool: its schedule is cyclic, which isim_des_workers_set refuses.)"""
    workers = GRAPHS["zero_hold"][5]
    c, r, s = check("zero_hold", workers, SBK)
    names = [x["name"] for x in c.h.graph.canonical()["services"]]
    w = s["start_ns"] > s["arrival_ns"]
    assert np.any(w & (s["service"] == names.index("b"))) and not np.any(w & (s["service"] == names.index("z")))
    # every round is sort-free: the item count, the buckets and the fault word are all the host reads back
    c.d.serve(BEGIN, GRAPHS["zero_hold"][4])
    assert c.d.last_batch()["syncs"] == 3
    _, r0, s0 = device("zero_hold", workers, 0)
    assert np.array_equal(s0, s)
    for f in ("recs", "stats", "table", "wait"):
        assert np.array_equal(r0[f], r[f]), f


SOURCES = [("prob", BEGIN, None), ("modeb", BEGIN, None), ("wide", BEGIN, None), ("t64", BEGIN, None),
           ("prob", (1 << 32) - 300, 601), ("mixed", (1 << 32) - 300, 601)]


@pytest.mark.parametrize("name,begin,n", SOURCES, ids=[f"{g}-{b}" for g, b, _ in SOURCES])
def test_order_sources_scans_and_sorts_agree(gpu, name, begin, n):
    workers = GRAPHS[name][5]
    c, r, s = check(name, workers, 0, begin, n)
    for flags in (SBK, TWO, SBK | TWO):
        _, r2, s2 = device(name, workers, flags, begin, n)
        assert np.array_equal(s2, s), flags
        for f in ("recs", "stats", "table", "wait"):
            assert np.array_equal(r2[f], r[f]), (flags, f)


def test_ties_under_a_paced_load(gpu):
    c, r, s = check("ties_paced", GRAPHS["ties_paced"][5], paced=True)
    assert np.array_equal(s["arrival_ns"][s["hop"] == 0], paced_arrivals(200_000, GRAPHS["ties_paced"][4]))
    _, r2, s2 = device("ties_paced", GRAPHS["ties_paced"][5], SBK | TWO, paced=True)
    assert np.array_equal(s2, s)


def test_ties_at_a_gap_of_one_ns(gpu):
    c, r, s = check("ties_fanout", GRAPHS["ties_fanout"][5])
    _, r2, s2 = device("ties_fanout", GRAPHS["ties_fanout"][5], TWO)
    assert np.array_equal(s2, s)


@pytest.mark.parametrize("name", ["two", "mixed", "prob"])
def test_all_ones_is_the_untouched_handler(gpu, name):
    doc, mode, kw, mean, n, _ = GRAPHS[name]
    never, ones = DesCase(doc(), mean, error_mode=mode, **kw), DesCase(doc(), mean, error_mode=mode, **kw)
    ones.d.workers = 1
    a, b = never.d.serve(BEGIN, n), ones.d.serve(BEGIN, n)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert never.d.workspace_bytes(n) == ones.d.workspace_bytes(n)
    assert never.d.last_batch() == ones.d.last_batch()
    # and pooled, then back to 1: the same bytes again
    ones.d.workers = 2
    assert ones.d.serve(BEGIN, n)[0].tobytes() != a[0].tobytes()
    ones.d.workers = None
    for x, y in zip(a, ones.d.serve(BEGIN, n)):
        assert x.tobytes() == y.tobytes()


def test_service_timeline_and_critical_path_over_a_pooled_batch(gpu):
    name, W = "prob", 3
    c = case(name)
    n = GRAPHS[name][4]
    d = c.d
    d.workers = W
    want = reference(name, W)
    hold = np.array(ref.holds(c.sg), np.uint64)
    count = np.bincount(want["service"], minlength=len(hold)).astype(np.uint64)
    window = 1_000_000
    n_windows = int(want["finish_ns"].max()) // window + 2
    t = d.service_timeline(BEGIN, n, window, n_windows)
    assert t.workers.tolist() == [W] * len(hold) and t.header == dict(folded=len(want), refused=0)
    assert np.array_equal(t.table[:, :, native.SVT_BUSY_NS].sum(axis=1, dtype=np.uint64), count * hold)
    assert np.array_equal(t.table[:, :, native.SVT_SUM_WAIT].sum(axis=1, dtype=np.uint64),
                          ref.table_of(want, len(hold))[:, 1])
    u = t.utilisation()
    assert float(u.max()) <= 1.0 and float(u.max()) > 1.0 / W   # more than one worker of some replica was busy
    assert "workers" in t.to_text().splitlines()[1]
    recs, stats, table, traces, waits, path = d.serve_spans(BEGIN, n, min_latency_ns=0, max_traces=n,
                                                            cap_spans=len(want), critical_path=True)
    assert len(traces) == n and np.array_equal(recs["latency_ns"], ref.latencies(want))
    ns = c.h.info.n_services
    pt = path.table
    part = pt[:ns, native.DCP_WAIT_NS] + pt[:ns, native.DCP_SELF_NS] + pt[:ns, native.DCP_HOP_NS]
    assert int(part.sum(dtype=np.uint64)) == int(pt[ns, native.DCP_H_SUM_LATENCY]) == int(recs["latency_ns"].sum())
    assert path.header["refused"] == 0 and int(pt[:ns, native.DCP_WAIT_NS].sum()) > 0
