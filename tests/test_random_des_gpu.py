"""GPU parity of the DES on seeded random graphs over the schema's whole
vocabulary (tests/random_des_graphs.py): both engines, acyclic and cyclic
schedules, against the event-driven C oracle on 1,100 traces — records, folded
stats and the DES table, bit-exact, in both error modes; the level engine's
narrow and wide rows against each other; the item engine's scans and sorts
against each other; level-class graphs forced onto the item engine against the
level engine; the span tap, the DES critical path and the service timeline of
the item engine against the Python restatement on 293 traces; and worker pools
against the pooled restatement.  tests/test_random_des.py pins the family, the
classes and the references on the same seeds without a GPU.  A case the host
refuses (no unrolled tree under a dynamic walk) asserts the refusal."""
import numpy as np
import pytest

import isim
from isim import native

import des_spans_ref as ref
import random_des_graphs as rd
import random_walk_graphs as rw
from test_des_spans_gpu import NONE, run_tap
from test_des_workers_gpu import at_most_w_busy, equals_the_restatement

pytestmark = pytest.mark.gpu

SBK, TWO, ALL = native.FLAG_DES_SCAN_BY_KEY, native.FLAG_DES_TWO_SORTS, native.FLAG_DES_SORT_ALL
ITEM_FLAGS = (SBK, TWO | SBK, ALL)
FIELDS = ("arrival_ns", "start_ns", "finish_ns", "hop_ns", "hop", "caller_hop", "position", "service", "status",
          "replica")
STAT_KEYS = ("n_traces", "sum_latency", "sum_hops", "sum_err_hops", "n_500", "max_latency", "min_latency")
STAT_ARRAYS = ("lat_prom", "lat_log2", "svc_calls", "svc_errs", "site_calls")


class _WideRows:
    """A DesHandler whose device batches run with 64-bit rows (run_tap asks for the default, 32-bit)."""

    def __init__(self, d):
        self._d = d

    def __getattr__(self, name):
        return getattr(self._d, name)

    def serve_spans_device(self, *args, **kw):
        return self._d.serve_spans_device(*args, wide=True, **kw)


def tapped(c):
    """The whole N_SPANS window of `c` tapped (threshold 0, every trace, room for every span): (buffers, spans).
    The item engine keeps 64-bit times whatever the rows (127 of the 174 cases have a latency past 2^31 ns
    on this window); a batch it does drop — counted, nothing written — is served again with 64-bit rows."""
    n = rd.N_SPANS
    r = run_tap(c, c.begin, n)
    dropped = int(r["stats"][native.ST_DES_RETRY])
    if dropped:
        assert dropped == 1 and int(r["stats"][native.ST_N_TRACES]) == 0
        assert int(r["info"][native.SPAN_WRITTEN]) == 0 and int(r["off"][0]) == 0 and not r["wait"].any()
        r = run_tap(c, c.begin, n, d=_WideRows(c.d))
        assert int(r["stats"][native.ST_DES_RETRY]) == 0
    total = int(r["off"][n])
    assert list(r["info"]) == [total, n, n, n, n]
    assert np.array_equal(r["ids"], np.arange(c.begin, c.begin + n, dtype=np.uint64))
    return r, r["spans"][:total]


def assert_spans_equal(c, r, s, want):
    """test_des_spans_gpu.test_spans_equal_the_restatement on the case's window."""
    n = rd.N_SPANS
    assert len(s) == len(want)
    assert np.array_equal(np.diff(r["off"][:n + 1].astype(np.int64)), r["recs"]["hops"])
    assert np.array_equal(r["recs"]["hops"], np.bincount((want["trace"] - np.uint64(c.begin)).astype(np.int64), minlength=n))
    for f in FIELDS:
        bad = np.flatnonzero(s[f] != want[f])
        assert bad.size == 0, (f, bad[:4], s[bad[:4]], want[bad[:4]])
    entry = s["hop"] == 0
    assert np.all(s["slot"][entry] == NONE) and not s["reserved"].any()
    assert np.array_equal(c.h.slot_site[s["slot"][~entry]], want["site"][~entry].astype(np.int32))


def assert_wait_table(c, r, s):
    """test_des_spans_gpu.test_whole_batch_table_equals_the_des_table."""
    rows = c.d.fold(r["table"])
    ns = c.h.info.n_services
    wt = r["wait"]
    assert np.array_equal(wt[:ns, native.DW_INVOCATIONS], rows[:, native.DES_COUNT])
    assert np.array_equal(wt[:ns, native.DW_SUM_WAIT], rows[:, native.DES_SUM_WAIT])
    assert np.array_equal(wt[:ns, native.DW_MAX_WAIT], rows[:, native.DES_MAX_WAIT])
    assert np.array_equal(wt[:ns, native.DW_SUM_DURATION], rows[:, 2 * native.N_PROM] + rows[:, 2 * native.N_PROM + 1])
    w = s["start_ns"] - s["arrival_ns"]
    assert np.array_equal(wt[:ns, native.DW_WAITED], np.bincount(s["service"][w > 0], minlength=ns))
    assert np.array_equal(wt[:ns, native.DW_RESP_500], np.bincount(s["service"][(s["status"] & 1) == 1], minlength=ns))
    entry = s["hop"] == 0
    assert list(wt[ns]) == [rd.N_SPANS, len(s), int(r["recs"]["latency_ns"].sum()), int(w[entry].sum()), 0, 0]


def assert_invariants(c, r, s):
    """test_des_spans_gpu.test_invariants_on_every_span: on the device's spans alone."""
    n = rd.N_SPANS
    a, S, F = s["arrival_ns"], s["start_ns"], s["finish_ns"]
    assert np.all(a <= S) and np.all(S <= F)
    first = r["off"][:n].astype(np.int64)
    trace = np.repeat(np.arange(n), np.diff(r["off"][:n + 1].astype(np.int64)))
    child = s["hop"] != 0
    caller = first[trace[child]] + s["caller_hop"][child].astype(np.int64)
    assert np.all(a[child] >= S[caller] + s["hop_ns"][child]) and np.all(F[child] <= F[caller])
    assert np.array_equal(F[first] - a[first], r["recs"]["latency_ns"])
    assert np.array_equal(a[first], c.d.arrivals(c.begin, n))
    # one worker per (service, replica): the holds [S, S + P_s) do not overlap and start in (a, trace, hop) order
    hold = np.array(ref.holds(c.sg), np.uint64)[s["service"]]
    order = np.lexsort((s["hop"], trace, a, s["replica"], s["service"]))
    same = (s["service"][order][1:] == s["service"][order][:-1]) & (s["replica"][order][1:] == s["replica"][order][:-1])
    So, ho = S[order], hold[order]
    assert np.all(So[1:][same] >= (So[:-1] + ho[:-1])[same])


def assert_timeline_and_critical_path(c, r, want):
    """The folds of test_des_workers_gpu.test_service_timeline_and_critical_path_over_a_pooled_batch over
    the tapped batch: DesHandler.serve_spans(critical_path=True) and DesHandler.service_timeline."""
    n, ns = rd.N_SPANS, c.h.info.n_services
    hold = np.array(ref.holds(c.sg), np.uint64)
    count = np.bincount(want["service"], minlength=ns).astype(np.uint64)
    recs, stats, table, traces, waits, path = c.d.serve_spans(c.begin, n, min_latency_ns=0, max_traces=n,
                                                               cap_spans=len(want), critical_path=True)
    assert len(traces) == n and np.array_equal(recs, r["recs"])
    pt = path.table
    part = pt[:ns, native.DCP_WAIT_NS] + pt[:ns, native.DCP_SELF_NS] + pt[:ns, native.DCP_HOP_NS]
    assert int(part.sum(dtype=np.uint64)) == int(pt[ns, native.DCP_H_SUM_LATENCY]) == int(recs["latency_ns"].sum())
    assert path.header["refused"] == 0
    assert np.array_equal(waits.table, r["wait"])
    # windows of 1 ms; what lies past them is in the table's last row
    t = c.d.service_timeline(c.begin, n, 1_000_000, 64)
    assert t.header == dict(folded=len(want), refused=0)
    assert np.array_equal(t.table[:, :, native.SVT_BUSY_NS].sum(axis=1, dtype=np.uint64), count * hold)
    waited = t.table[:, :, native.SVT_SUM_WAIT].sum(axis=1, dtype=np.uint64)
    assert np.array_equal(waited, r["wait"][:ns, native.DW_SUM_WAIT])
    assert np.array_equal(waited, ref.table_of(want, ns)[:, 1])


# ---- a. both engines against the event-driven oracle

@pytest.mark.parametrize("family,seed", rd.CASES, ids=rd.IDS)
def test_engines_match_the_oracle(gpu, family, seed):
    for mode in rd.MODES:
        want = rd.census()[family, seed, mode]
        if rd.expected_refusal(family, seed, mode):
            assert want is None
            rd.assert_refused(family, seed, mode)
            continue
        c = rd.RandomDesCase(family, seed, mode)
        assert c.key() == want, (mode, c.key(), want)
        recs, stats, rows = c.compare(c.begin, rd.N_ORACLE)
        if not c.d.info.items:   # the level engine: 32-bit rows (wide on retry) and 64-bit rows
            r2, s2, rows2 = c.compare(c.begin, rd.N_ORACLE, wide=True)
            assert np.array_equal(recs, r2) and np.array_equal(stats, s2) and np.array_equal(rows, rows2), mode
            continue
        assert c.d.last_batch()["items"] == int(recs["hops"].sum())
        base = c.d.serve(c.begin, rd.N_ORACLE)
        assert np.array_equal(base[0], recs) and np.array_equal(base[1], stats), mode
        assert np.array_equal(c.d.fold(base[2]), rows), mode
        for flags in ITEM_FLAGS:   # each scan, each sort, kept orders or none: the same batch
            v = rd.RandomDesCase(family, seed, mode, flags)
            assert v.key() == want
            got = v.d.serve(c.begin, rd.N_ORACLE)
            for x, y, what in zip(got, base, ("records", "stats", "table")):
                assert np.array_equal(x, y), (mode, flags, what)


# ---- b. level-class graphs as dynamic walks: the item engine against the level engine and the oracle

@pytest.mark.parametrize("seed", rw.SEEDS)
def test_level_class_on_the_item_engine(gpu, seed):
    ran = 0
    for mode in rd.MODES:
        key = rd.census()["static", seed, mode]
        if key is None or key[0] == 1:
            continue
        ran += 1
        if rd.expected_refusal("static", seed, mode, native.FLAG_DYNAMIC):
            rd.assert_refused("static", seed, mode, native.FLAG_DYNAMIC)
            continue
        cs, cd = rd.RandomDesCase("static", seed, mode), rd.RandomDesCase("static", seed, mode, native.FLAG_DYNAMIC)
        assert cs.d.info.items == 0 and cd.d.info.items == 1
        rs, ss, ts = cs.compare(cs.begin, rd.N_ORACLE)
        ri, si, ti = cd.compare(cd.begin, rd.N_ORACLE)
        assert np.array_equal(rs, ri), mode
        fs, fi = cs.h.fold(ss), cd.h.fold(si)
        for k in STAT_KEYS:
            assert fs[k] == fi[k], (mode, k)
        for k in STAT_ARRAYS:
            assert np.array_equal(np.asarray(fs[k], np.uint64), np.asarray(fi[k], np.uint64)), (mode, k)
        assert np.array_equal(ts, ti), mode
    assert ran >= 1   # every static graph is level-class in mode A


# ---- c. the item engine's span tap against the restatement

@pytest.mark.parametrize("family,seed", rd.CASES, ids=rd.IDS)
def test_tap_equals_the_restatement(gpu, family, seed):
    for mode in rd.MODES:
        key = rd.census()[family, seed, mode]
        if key is None or key[0] == 0:
            continue
        c = rd.RandomDesCase(family, seed, mode)
        want = rd.reference(family, seed, mode)
        r, s = tapped(c)
        assert_spans_equal(c, r, s, want)
        assert_wait_table(c, r, s)
        assert_invariants(c, r, s)
        if seed % 4 == 1:   # a forced wide tree: 16-byte nodes in the pre-walk, the same spans
            v = rd.RandomDesCase(family, seed, mode, native.FLAG_TREE_WIDE)
            assert v.h.launch_info(0)["tree_wide"] == 1
            r2, s2 = tapped(v)
            assert_spans_equal(v, r2, s2, want)
            for f in ("recs", "stats", "table", "wait"):
                assert np.array_equal(r2[f], r[f]), (mode, f)
        assert_timeline_and_critical_path(c, r, want)


# ---- d. worker pools against the pooled restatement

@pytest.mark.parametrize("family,seed,mode", rd.POOLED, ids=rd.POOLED_IDS)
def test_pools_equal_the_pooled_restatement(gpu, family, seed, mode):
    n = rd.N_SPANS
    never = rd.RandomDesCase(family, seed, mode)
    assert never.key()[:2] == (1, 0)
    untouched = never.d.serve(never.begin, n)
    c = rd.RandomDesCase(family, seed, mode)   # its own handler: the pool is the handler's state
    wl = rd.pool(seed, c.h.info.n_services)
    c.d.workers = wl
    assert c.d.workers.tolist() == wl
    want = rd.pooled_reference(family, seed, mode)
    r, s = tapped(c)
    equals_the_restatement(c, r, s, want)
    at_most_w_busy(c, s, wl)
    v = rd.RandomDesCase(family, seed, mode, SBK | TWO)
    v.d.workers = wl
    r2, s2 = tapped(v)
    assert np.array_equal(s2, s)
    for f in ("recs", "stats", "table", "wait"):
        assert np.array_equal(r2[f], r[f]), f
    c.d.workers = None
    assert c.d.workers.tolist() == [1] * len(wl)
    for x, y in zip(untouched, c.d.serve(c.begin, n)):
        assert x.tobytes() == y.tobytes()


# ---- e. the classes, on the machine the kernels run on

def test_engine_census(gpu):
    """Handlers only, no launch: the class counts of tests/test_random_des.py::test_class_census, the pooled
    cases, and that the parametrisations above leave no accepted case out."""
    cen = rd.census()
    rd.check_census_counts(cen)
    assert rd.pooled_cases() == rd.POOLED and len(rd.POOLED) == 15
    accepted = {k for k, v in cen.items() if v is not None}
    assert {(f, s, m) for f, s in rd.CASES for m in rd.MODES} == set(cen)
    in_b = {k for k in accepted if k[0] == "static" and cen[k][0] == 0}
    in_c = {k for k in accepted if cen[k][0] == 1}
    assert len(accepted) == 174 and len(in_b) == 72 and len(in_c) == 102 and in_b | in_c >= \
        {k for k in accepted if k[0] == "static"}
