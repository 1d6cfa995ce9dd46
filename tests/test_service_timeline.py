"""The service timeline on the CPU: isim_service_timeline_host against hand-derived
vectors and, word for word, against a naive restatement (tests/service_timeline_ref.py) on the Python
reference spans of three graphs; the identities of a zeroed table; refused spans; accumulation and merge;
every argument the entry points refuse, found on the host before any HIP call; the services' holds."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import isim
from isim import native
from isim.yamljson import obj_to_json

import des_spans_ref as dref
import service_timeline_ref as ref
from test_des_spans import case_of, reference

MEAN = 300_000
GRAPHS = [("canonical_p50", isim.MODE_A), ("tree_reps_p70", isim.MODE_A), ("zero_hold_mix", isim.MODE_A)]
# (window_ns, n_windows): 1 ns, 1 us, a window that is no power of two, 2^40
WINDOWS = [(1, 4096), (1000, 4096), (333_333, 300), (1 << 40, 3)]
W = native.SVT_ROW_WORDS
KAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "service_timeline_kat.json")


def des_spans(rows) -> np.ndarray:
    """Reference rows (des_spans_ref.REF_DTYPE) as isim_des_span records."""
    out = np.zeros(len(rows), isim.DES_SPAN_DTYPE)
    for f in ("arrival_ns", "start_ns", "finish_ns", "hop_ns", "hop", "caller_hop", "position", "service", "status",
              "replica"):
        out[f] = rows[f]
    return out


@functools.lru_cache(maxsize=None)
def spans_of(name, mode):
    s = des_spans(reference(name, mode, MEAN))
    s.setflags(write=False)
    return s


def rows_of(flat, ns):
    return flat[:-W].reshape(ns, -1, W)


@functools.lru_cache(maxsize=None)
def one_service(hold_ns=5):
    doc = {"services": [{"name": "a", "isEntrypoint": True, "script": [{"sleep": f"{hold_ns}ns"}]}]}
    return isim.Handler(isim.ServiceGraph.from_json(obj_to_json(doc)), None, isim.SimParams(flags=native.FLAG_DYNAMIC))


def kat_cases():
    return json.load(open(KAT))["cases"]


@pytest.mark.parametrize("case", kat_cases(), ids=[c["name"] for c in kat_cases()])
def test_hand_derived_vectors(case):
    h = one_service(case["hold"])
    spans = np.zeros(len(case["spans"]), isim.DES_SPAN_DTYPE)
    for i, (a, S, F, st) in enumerate(case["spans"]):
        spans[i]["arrival_ns"], spans[i]["start_ns"], spans[i]["finish_ns"], spans[i]["status"] = a, S, F, st
    n = case["n_windows"]
    want = np.zeros((n + 3) * W, np.uint64)
    for row, word, value in case["cells"]:
        want[row * W + word] = value
    want[(n + 2) * W + native.SVT_H_FOLDED], want[(n + 2) * W + native.SVT_H_REFUSED] = case["header"]
    got = isim.service_timeline_host(h, spans, case["window"], n, case["t0"])
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    # the naive restatement agrees with the hand derivation too
    assert np.array_equal(ref.fold_exact(spans, 1, [case["hold"]], case["window"], n, case["t0"]), want)
    # over all rows the overlaps of an interval sum to its length
    t = rows_of(got, 1)[0]
    waits = sum(S - a for a, S, _, _ in case["spans"])
    busy = sum(min(S + case["hold"], ref.M64) - S for _, S, _, _ in case["spans"])
    assert sum(int(x) for x in t[:, native.SVT_QUEUED_NS]) == waits == sum(int(x) for x in t[:, native.SVT_SUM_WAIT])
    assert sum(int(x) for x in t[:, native.SVT_BUSY_NS]) == busy


def t0_of(spans, mid):
    return int(np.sort(spans["arrival_ns"])[len(spans) // 2]) if mid else 0


@pytest.mark.parametrize("mid", [False, True], ids=["t0=0", "t0=mid"])
@pytest.mark.parametrize("window", WINDOWS, ids=[f"w{w[0]}" for w in WINDOWS])
@pytest.mark.parametrize("graph", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_equals_the_naive_restatement(graph, window, mid):
    c = case_of(*graph, MEAN)
    s = spans_of(*graph)
    ns = c.h.info.n_services
    t0 = t0_of(s, mid)
    got = isim.service_timeline_host(c.h, s, window[0], window[1], t0)
    want = ref.fold(s, ns, dref.holds(c.sg), window[0], window[1], t0)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:4], got[bad[:4]], want[bad[:4]])


def check_identities(flat, spans, ns, hold):
    """The per-service identities of a zeroed table over spans none of which is refused."""
    t = rows_of(flat, ns)
    wait = spans["start_ns"] - spans["arrival_ns"]
    for s in range(ns):
        m = spans["service"] == s
        cnt = int(m.sum())
        assert int(t[s, :, native.SVT_ARRIVED].sum()) == int(t[s, :, native.SVT_STARTED].sum()) == cnt
        assert int(t[s, :, native.SVT_FINISHED:native.SVT_FINISHED + 2].sum()) == cnt
        total = int(wait[m].sum())
        assert int(t[s, :, native.SVT_SUM_WAIT].sum()) == int(t[s, :, native.SVT_QUEUED_NS].sum()) == total
        assert int(t[s, :, native.SVT_BUSY_NS].sum()) == cnt * int(hold[s])
        assert int(t[s, :, native.SVT_MAX_WAIT].max()) == (int(wait[m].max()) if cnt else 0)
        depth = np.cumsum(t[s, :, native.SVT_ARRIVED].astype(np.int64)) - np.cumsum(t[s, :, native.SVT_STARTED].astype(np.int64))
        assert depth.min() >= 0 and depth[-1] == 0
    assert list(flat[-W:]) == [len(spans), 0] + [0] * (W - 2)


@pytest.mark.parametrize("graph", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_identities_per_service(graph):
    c = case_of(*graph, MEAN)
    s = spans_of(*graph)
    ns = c.h.info.n_services
    hold = dref.holds(c.sg)
    for window, n in WINDOWS:
        for mid in (False, True):
            check_identities(isim.service_timeline_host(c.h, s, window, n, t0_of(s, mid)), s, ns, hold)
    t = isim.ServiceTimeline(c.h, 333_333, 300, 0, isim.service_timeline_host(c.h, s, 333_333, 300, 0))
    assert t.header == {"folded": len(s), "refused": 0}
    assert np.array_equal(t.queue_depth()[:, -1], np.zeros(ns, np.uint64))
    reps = np.array([max(1, x.num_replicas) for x in c.sg.g.services])
    assert np.array_equal(t.replicas, reps) and t.utilisation().shape == t.mean_queue().shape == (ns, 300)
    # one worker per replica: no window is busier than window x replicas
    assert np.all(t.table[:, 1:-1, native.SVT_BUSY_NS] <= np.uint64(333_333) * reps[:, None].astype(np.uint64))
    assert 0.0 < t.utilisation().max() <= 1.0
    text = t.to_text(top=2).splitlines()
    assert len(text) == 4 and text[0].startswith(f"service timeline of {len(s)} spans")


def test_refused_spans_count_in_the_header_only():
    graph = GRAPHS[2]
    c = case_of(*graph, MEAN)
    good = spans_of(*graph)[:500]
    ns = c.h.info.n_services
    bad = good[:60].copy()
    bad["service"][:20] = ns                               # a service out of range
    bad["service"][10:20] = 0xFFFFFFFF
    bad["start_ns"][20:40] = bad["arrival_ns"][20:40] - 1   # S < a
    bad["finish_ns"][40:60] = bad["start_ns"][40:60] - 1    # F < S
    mixed = np.concatenate([bad[:30], good, bad[30:]])
    want = isim.service_timeline_host(c.h, good, 1000, 4096, 0)
    want[-W + native.SVT_H_REFUSED] = 60
    assert np.array_equal(isim.service_timeline_host(c.h, mixed, 1000, 4096, 0), want)
    assert np.array_equal(ref.fold_exact(mixed[:90], ns, dref.holds(c.sg), 1 << 40, 3, 0),
                          isim.service_timeline_host(c.h, mixed[:90], 1 << 40, 3, 0))


def test_a_nonzero_table_and_merge():
    graph = GRAPHS[1]
    c = case_of(*graph, MEAN)
    s = spans_of(*graph)
    half = len(s) // 2
    window, n, t0 = 333_333, 300, t0_of(s, True)
    a, b = (isim.service_timeline_host(c.h, part, window, n, t0) for part in (s[:half], s[half:]))
    rng = np.random.default_rng(7)
    start = rng.integers(1, 1 << 30, a.size, dtype=np.uint64)
    mx = np.zeros(a.size, bool)
    mx[:-W][native.SVT_MAX_WAIT::W] = True
    start[mx] = a[mx] // 2 + 1   # some maxima win, some lose
    # the fold adds into what is there, calling again is the device's merge ...
    acc = isim.service_timeline_host(c.h, s[:half], window, n, t0, table=start.copy())
    acc = isim.service_timeline_host(c.h, s[half:], window, n, t0, table=acc)
    want = start + a + b
    want[mx] = np.maximum(np.maximum(start[mx], a[mx]), b[mx])
    assert np.array_equal(acc, want)
    # ... and isim_service_timeline_merge does the same on the host, the MAX word included
    ta, tb = (isim.ServiceTimeline(c.h, window, n, t0, x.copy()) for x in (start, a))
    assert ta.merge(tb) is ta and np.array_equal(tb.flat, a)
    ta.merge(isim.ServiceTimeline(c.h, window, n, t0, b))
    assert np.array_equal(ta.flat, want)
    # both halves in one call: the whole batch
    whole = isim.service_timeline_host(c.h, s, window, n, t0)
    both = a + b
    both[mx] = np.maximum(a[mx], b[mx])
    assert np.array_equal(whole, both)


def test_service_holds():
    for graph in GRAPHS:
        c = case_of(*graph, MEAN)
        hold, reps = isim.service_holds(c.h)
        assert list(hold) == dref.holds(c.sg)
        assert list(reps) == [max(1, x.num_replicas) for x in c.sg.g.services]
    assert max(isim.service_holds(case_of(*GRAPHS[1], MEAN).h)[1]) > 1      # a replicated service
    assert min(isim.service_holds(case_of(*GRAPHS[2], MEAN).h)[0]) == 0     # P_s = 0


def _einval(rc, match):
    assert rc == native.EINVAL and match in native.last_error(), native.last_error()


def test_refusals_need_no_gpu():
    lib = native.load()
    items = one_service()
    static_doc = {"services": [{"name": "a", "isEntrypoint": True, "script": [{"sleep": "1ms"}, {"call": "b"}]},
                               {"name": "b", "script": [{"sleep": "1ms"}]}]}
    static = isim.Handler(isim.ServiceGraph.from_json(obj_to_json(static_doc)), None, isim.SimParams())
    many = {"services": [{"name": f"s{i}", "isEntrypoint": i == 0} for i in range(300)]}
    wide = isim.Handler(isim.ServiceGraph.from_json(obj_to_json(many)), None, isim.SimParams(flags=native.FLAG_DYNAMIC))
    buf = np.zeros(64, np.uint64)   # never dereferenced by a refused call
    a = buf.ctypes.data
    assert a % 16 == 0
    P = native.TimelineParams
    ok = P(0, 1000, 8, 0)
    out = C.c_uint64()

    def every(h, p):
        """Every entry point that takes the handler and the parameters."""
        q = C.byref(p) if p is not None else None
        hh = h._h if h is not None else None
        return [lib.isim_service_timeline_table_words(hh, q, C.byref(out)),
                lib.isim_service_timeline_workspace_bytes(hh, q, C.byref(out)),
                lib.isim_service_timeline_merge(hh, q, a, a),
                lib.isim_service_timeline_host(hh, q, a, 1, a),
                lib.isim_service_timeline(0, hh, q, a, 1, a),
                lib.isim_service_timeline_device(hh, q, a, a, 1, a, a, a, 1 << 30, None)]

    for why, h, p in [("null handler", None, ok), ("ISIM_FLAG_DYNAMIC", static, ok), ("null isim_timeline_params", items, None),
                      ("window_ns", items, P(0, 0, 8, 0)), ("n_windows", items, P(0, 1000, 0, 0)),
                      ("n_windows", items, P(0, 1000, 65537, 0)), ("reserved", items, P(0, 1000, 8, 1)),
                      ("2^24", wide, P(0, 1000, 65536, 0))]:
        for rc in every(h, p):
            _einval(rc, why)
    assert lib.isim_service_timeline_table_words(wide._h, C.byref(P(0, 1000, 50000, 0)), C.byref(out)) == native.OK
    assert out.value == (300 * 50002 + 1) * W
    q = C.byref(ok)
    assert lib.isim_service_timeline_table_words(items._h, q, C.byref(out)) == native.OK and out.value == 11 * W
    assert lib.isim_service_timeline_workspace_bytes(items._h, q, C.byref(out)) == native.OK and out.value == 160
    _einval(lib.isim_service_timeline_table_words(items._h, q, None), "null")
    _einval(lib.isim_service_timeline_workspace_bytes(items._h, q, None), "null")
    _einval(lib.isim_service_timeline_merge(items._h, q, a, None), "null")
    _einval(lib.isim_service_timeline_merge(items._h, q, None, a), "null")
    _einval(lib.isim_des_service_holds(None, a, a), "null handler")
    _einval(lib.isim_des_service_holds(static._h, a, a), "ISIM_FLAG_DYNAMIC")
    _einval(lib.isim_des_service_holds(items._h, None, a), "null")
    _einval(lib.isim_des_service_holds(items._h, a, None), "null")
    for call in (lambda *x: lib.isim_service_timeline_host(items._h, q, *x),
                 lambda *x: lib.isim_service_timeline(0, items._h, q, *x)):
        _einval(call(a, (1 << 40) + 1, a), "2^40")
        _einval(call(a, 1, None), "null table")
        _einval(call(None, 1, a), "null spans")
    _einval(lib.isim_service_timeline_host(items._h, q, a, 1, a + 4), "aligned")

    def dev(off=a, spans=a, cap=4, info=a, table=a, ws=a, ws_bytes=1 << 30):
        return lib.isim_service_timeline_device(items._h, q, off, spans, cap, info, table, ws, ws_bytes, None)

    _einval(dev(cap=(1 << 40) + 1), "2^40")
    for null in ("off", "info", "table", "spans"):
        _einval(dev(**{null: None}), "null")
    for mis in ("off", "info", "table", "ws"):
        _einval(dev(**{mis: a + 4}), "aligned")
    _einval(dev(spans=a + 8), "aligned")
    _einval(dev(ws_bytes=159), "workspace")
    _einval(dev(ws=None), "workspace")
    with pytest.raises(isim.IsimError) as e:
        isim.DesHandler(static, 300_000).service_timeline(0, 8, 1000, 8)
    assert e.value.code == native.EINVAL
