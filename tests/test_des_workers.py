"""DES worker pools on the CPU: the two declarations and
their round trips, every refusal (found on the host before any HIP call), the
Python side, and the reference the GPU tests check against
(tests/des_workers_ref.py): pinned to the one-worker restatement, checked
against the stride recurrence the device solves, against the plain walk when
nobody waits, and shown to be contended on every graph and gap the GPU tests
use.  Also the class layout's index formula (csrc/des_workers.h) as a
permutation."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

import isim
from isim import native
from isim.generators import tree_topology
from isim.yamljson import obj_to_json
from oracle import executor as oc

import des_spans_ref as ref1
import des_workers_ref as ref
from test_des_gpu import DesCase, _sleepy_tree
from test_des_items_gpu import CASES, _err, _sleepy, _with_prob
from test_des_spans import ALL, case_of as spans_case, invocations_of as spans_invocations, reference as spans_reference

DYN = native.FLAG_DYNAMIC


def _two(reps=1):
    """Every trace calls one sleeping service: its queue is one segment of n items per replica."""
    return {"services": [{"name": "a", "isEntrypoint": True, "script": [{"call": "b"}]},
                         {"name": "b", "numReplicas": reps, "script": [{"sleep": "2ms"}]}]}


def _mixed():
    """b, c and z arrive in one round (a's call step), d from two positions; z holds no worker."""
    return {"services": [
        {"name": "a", "isEntrypoint": True, "numReplicas": 2,
         "script": [{"sleep": "200us"}, [{"call": {"service": "b", "probability": 60}},
                                         {"call": {"service": "c", "probability": 60}}, {"call": "z"}]]},
        {"name": "b", "script": [{"sleep": "700us"}, {"call": "d"}]},
        {"name": "c", "script": [{"sleep": "300us"}, {"call": {"service": "d", "probability": 50}}]},
        {"name": "d", "script": [{"sleep": "400us"}]},
        {"name": "z"}]}


def _zero_hold():
    """b and the sleep-free z arrive in one round, a's call step, both in trace order behind a's one replica:
    a sort-free round (its list is its FIFO order) in which z's items are each a segment of their own next to
    b's one segment.  (The item suite's zero_hold_mix has a cyclic schedule, which takes no pools.)"""
    return {"services": [
        {"name": "a", "isEntrypoint": True,
         "script": [{"sleep": "200us"}, [{"call": {"service": "b", "probability": 50}}, {"call": "z"}]]},
        {"name": "b", "script": [{"sleep": "700us"}]},
        {"name": "z"}]}


def _ties_paced():
    """Zero hop cost and a paced load of one request per 200 us: b's arrivals through c of trace t - 1 and
    straight from a of trace t meet at the same instant, so (trace, hop) decides their ranks."""
    return {"services": [
        {"name": "a", "isEntrypoint": True, "script": [{"sleep": "100us"}, [{"call": "b"}, {"call": "c"}]]},
        {"name": "c", "script": [{"sleep": "200us"}, {"call": "b"}]},
        {"name": "b", "script": [{"sleep": "300us"}]}]}


def _ties_fanout():
    """20 calls of one trace reach z at one instant, and at a mean gap of 1 ns many traces start together."""
    return {"services": [
        {"name": "a", "isEntrypoint": True,
         "script": [{"sleep": "100us"}, [{"call": {"service": "z", "probability": 90}}] * 20]},
        {"name": "z", "script": [{"sleep": "10us"}]}]}


_PROB = lambda: _with_prob(_sleepy_tree(2, 3, reps_leaves=2), 70)  # noqa: E731
NOHOP = dict(hop_base_ns=0, req_ps_per_byte=0, resp_ps_per_byte=0)
# name: (document, error mode, SimParams arguments, mean gap ns, traces, workers as DesHandler takes them)
GRAPHS = {
    "two": (_two, isim.MODE_A, dict(flags=DYN), 1_000, 3000, 2),
    "two_reps": (lambda: _two(3), isim.MODE_A, dict(flags=DYN), 1_000, 3000, 2),
    "mixed": (_mixed, isim.MODE_A, {}, 150_000, 2500, {"b": 2, "d": 3, "z": 4}),
    "prob": (_PROB, isim.MODE_A, {}, 300_000, 2000, 2),
    "modeb": (lambda: _err(_sleepy(tree_topology(2, 3, sequential=True)), [0.15, 0.0, 0.3]), isim.MODE_B, {},
              150_000, 2000, 2),
    "wide": (_PROB, isim.MODE_A, dict(flags=native.FLAG_TREE_WIDE), 300_000, 2000, 3),
    "t64": (lambda: _with_prob(_sleepy(tree_topology(2, 3), pre="3s", post="1ms"), 70), isim.MODE_A, {},
            300_000, 2000, 2),
    "ties_paced": (_ties_paced, isim.MODE_A, dict(flags=DYN, **NOHOP), 200_000, 2000, {"b": 3}),
    "ties_fanout": (_ties_fanout, isim.MODE_A, {}, 1, 1500, {"a": 2, "z": 3}),
    "zero_hold": (_zero_hold, isim.MODE_A, {}, 150_000, 2500, {"b": 3}),
}
BEGIN = 1000


@functools.lru_cache(maxsize=None)
def case(name, extra_flags=0):
    doc, mode, kw, mean, _, _ = GRAPHS[name]
    kw = dict(kw)
    kw["flags"] = kw.get("flags", 0) | extra_flags
    return DesCase(doc(), mean, error_mode=mode, **kw)


def names_of(c):
    return [s["name"] for s in c.h.graph.canonical()["services"]]


def worker_list(c, workers):
    """Workers per service index from an int, a {name: k} dict or a list."""
    names = names_of(c)
    if isinstance(workers, dict):
        return [int(workers.get(nm, 1)) for nm in names]
    if np.ndim(workers) == 0:
        return [int(workers)] * len(names)
    return [int(w) for w in workers]


@functools.lru_cache(maxsize=None)
def invocations(name, begin, n):
    c = case(name)
    return ref.invocations(c.sg, c.op, begin, n)


@functools.lru_cache(maxsize=None)
def _reference(name, begin, n, wl, arr_key):
    c = case(name)
    arr = ref.arrivals(c.op.seed, GRAPHS[name][3], begin, n) if arr_key is None else np.array(arr_key, np.uint64)
    spans = ref.simulate(c.sg, c.op, begin, n, arr, wl, invocations(name, begin, n))
    spans.setflags(write=False)
    return spans


def reference(name, workers, begin=BEGIN, n=None, arr=None):
    """The pooled restatement's spans of one batch, computed once and never modified.  arr: the arrival times
    when they are not the constant mean's (a profile's)."""
    c = case(name)
    n = GRAPHS[name][4] if n is None else n
    return _reference(name, begin, n, tuple(worker_list(c, workers)), None if arr is None else tuple(int(a) for a in arr))


def paced_arrivals(mean, n):
    """A constant paced profile's arrivals: trace i of the batch at (i + 1) x mean."""
    return (np.arange(1, n + 1, dtype=np.uint64)) * np.uint64(mean)


# ---- the interface

def _handlers():
    items = case("mixed").h
    static = isim.Handler(isim.ServiceGraph.from_json(obj_to_json(_two())), None, isim.SimParams())
    cyclic = isim.Handler(isim.ServiceGraph.from_json(obj_to_json(CASES["zero_hold_mix"]())), None, isim.SimParams())
    return items, static, cyclic


def test_declarations_and_round_trips():
    assert native.SIGNATURES["isim_des_workers_set"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32])
    assert native.SIGNATURES["isim_des_workers_get"] == (C.c_int, [C.c_void_p, C.c_void_p])
    lib = native.load()
    assert lib.isim_abi_version() == 10
    h = isim.Handler(isim.ServiceGraph.from_json(obj_to_json(_mixed())), None, isim.SimParams())
    n = h.info.n_services
    got = np.zeros(n, np.uint32)
    native.check(lib.isim_des_workers_get(h._h, got.ctypes.data))
    assert got.tolist() == [1] * n                       # never set
    want = np.array([1, 2, 65536, 3, 4], np.uint32)
    native.check(lib.isim_des_workers_set(h._h, want.ctypes.data, n))
    native.check(lib.isim_des_workers_get(h._h, got.ctypes.data))
    assert np.array_equal(got, want)
    native.check(lib.isim_des_workers_set(h._h, None, n))   # NULL: every service back to 1
    native.check(lib.isim_des_workers_get(h._h, got.ctypes.data))
    assert got.tolist() == [1] * n
    # a refused set leaves the state as it was
    native.check(lib.isim_des_workers_set(h._h, want.ctypes.data, n))
    bad = np.array([1, 0, 1, 1, 1], np.uint32)
    assert lib.isim_des_workers_set(h._h, bad.ctypes.data, n) == native.EINVAL
    native.check(lib.isim_des_workers_get(h._h, got.ctypes.data))
    assert np.array_equal(got, want)


def test_python_workers():
    h = isim.Handler(isim.ServiceGraph.from_json(obj_to_json(_mixed())), None, isim.SimParams())
    d = isim.DesHandler(h, 150_000)
    assert d.workers.dtype == np.uint32 and d.workers.tolist() == [1] * 5
    assert isim.DesHandler(h, 150_000, workers=3).workers.tolist() == [3] * 5
    assert isim.DesHandler(h, 150_000, workers={"b": 2, "z": 4}).workers.tolist() == [1, 2, 1, 1, 4]
    assert isim.DesHandler(h, 150_000).workers.tolist() == [1, 2, 1, 1, 4]     # None: the handler's stay
    assert isim.DesHandler(h, 150_000, workers=np.array([5, 4, 3, 2, 1])).workers.tolist() == [5, 4, 3, 2, 1]
    d.workers = None
    assert d.workers.tolist() == [1] * 5
    with pytest.raises(ValueError):
        isim.DesHandler(h, 150_000, workers={"nobody": 2})
    for bad in (0, 65537, [1, 2, 3]):
        with pytest.raises(isim.IsimError) as e:
            isim.DesHandler(h, 150_000, workers=bad)
        assert e.value.code == native.EINVAL
    assert d.workers.tolist() == [1] * 5


def test_service_timeline_reads_the_workers():
    h = isim.Handler(isim.ServiceGraph.from_json(obj_to_json(_mixed())), None, isim.SimParams())
    W = native.SVT_ROW_WORDS
    words = isim.service_timeline_table_words(h, 1000, 2)
    flat = np.zeros(words, np.uint64)
    tab = flat[:-W].reshape(5, 4, W)
    tab[:, 1, native.SVT_BUSY_NS] = 1200
    tab[:, 1, native.SVT_ARRIVED] = 1
    one = isim.ServiceTimeline(h, 1000, 2, table=flat.copy())
    assert one.workers.tolist() == [1] * 5 and "workers" not in one.to_text()
    assert np.array_equal(one.utilisation()[:, 0], 1200 / (1000.0 * one.replicas))
    isim.DesHandler(h, 150_000, workers={"b": 2, "z": 4})
    t = isim.ServiceTimeline(h, 1000, 2, table=flat.copy())
    assert t.workers.tolist() == [1, 2, 1, 1, 4]
    assert np.array_equal(t.utilisation()[:, 0], 1200 / (1000.0 * t.replicas * np.array([1, 2, 1, 1, 4])))
    text = t.to_text().splitlines()
    assert "workers" in text[1] and len(text) == 2 + 5
    assert len(text[1]) == len(one.to_text().splitlines()[1]) + 8


def _einval(rc, match):
    assert rc == native.EINVAL and match in native.last_error(), native.last_error()


def test_refusals_need_no_gpu():
    lib = native.load()
    items, static, cyclic = _handlers()
    n = items.info.n_services
    w = lambda *v: np.array(v, np.uint32)  # noqa: E731
    try:
        _einval(lib.isim_des_workers_set(None, w(1).ctypes.data, 1), "null")
        _einval(lib.isim_des_workers_get(None, w(1).ctypes.data), "null")
        _einval(lib.isim_des_workers_get(items._h, None), "null")
        for h in (items, static, cyclic):   # the counts themselves, whatever the engine
            ns = h.info.n_services
            for bad in (0, 65537, 0xFFFFFFFF):
                v = np.ones(ns, np.uint32)
                v[ns - 1] = bad
                _einval(lib.isim_des_workers_set(h._h, v.ctypes.data, ns), "65536")
            for m in (ns - 1, ns + 1, 0):
                _einval(lib.isim_des_workers_set(h._h, np.ones(ns + 1, np.uint32).ctypes.data, m), "n_services")
        native.check(lib.isim_des_workers_set(items._h, w(1, 65536, 1, 2, 1).ctypes.data, n))
        # the level engine: no count above 1, and the message says how to get the item engine
        _einval(lib.isim_des_workers_set(static._h, w(1, 2).ctypes.data, 2), "ISIM_FLAG_DYNAMIC")
        native.check(lib.isim_des_workers_set(static._h, w(1, 1).ctypes.data, 2))
        # a cyclic call-step schedule: not built
        d = isim.DesHandler(cyclic, 300_000)
        assert d.info.items == 1 and d.info.cyclic == 1
        _einval(lib.isim_des_workers_set(cyclic._h, w(1, 2, 1, 1, 1).ctypes.data, 5), "cyclic")
        native.check(lib.isim_des_workers_set(cyclic._h, w(1, 1, 1, 1, 1).ctypes.data, 5))
        assert d.workers.tolist() == [1] * 5
    finally:
        lib.isim_des_workers_set(items._h, None, n)


# ---- the reference

@pytest.mark.parametrize("case_", ALL, ids=[c[0] for c in ALL])
def test_restatement_with_one_worker_is_the_spans_restatement(case_):
    _, name, mode = case_
    mean = 300_000
    c = spans_case(name, mode, mean)
    want = spans_reference(name, mode, mean)
    n = len(want[want["hop"] == 0])
    begin = int(want["trace"][0])
    got = ref.simulate(c.sg, c.op, begin, n, ref.arrivals(c.op.seed, mean, begin, n),
                       [1] * len(c.sg.g.services), spans_invocations(name, mode, begin, n))
    assert np.array_equal(got, want)


def _by_replica(spans):
    """The spans of each (service, replica) in FIFO order: (arrival, trace, hop)."""
    order = np.lexsort((spans["hop"], spans["trace"], spans["arrival_ns"], spans["replica"], spans["service"]))
    s = spans[order]
    cut = np.flatnonzero((s["service"][1:] != s["service"][:-1]) | (s["replica"][1:] != s["replica"][:-1])) + 1
    return np.split(s, cut)


RECURRENCE = [(g, w) for g in ("two_reps", "mixed", "prob", "modeb", "ties_fanout") for w in (2, 3, 64)]


@pytest.mark.parametrize("name,W", RECURRENCE, ids=[f"{g}-{w}" for g, w in RECURRENCE])
def test_restatement_satisfies_the_stride_recurrence(name, W):
    c = case(name)
    hold = ref.holds(c.sg)
    spans = reference(name, W)
    checked = 0
    for q in _by_replica(spans):
        a, S = q["arrival_ns"].astype(object), q["start_ns"].astype(object)
        P = hold[int(q["service"][0])]
        for j in range(len(q)):
            assert S[j] == (a[j] if j < W else max(a[j], S[j - W] + P)), (name, W, int(q["service"][0]), j)
        checked += max(0, len(q) - W)
    assert checked > 0


@pytest.mark.parametrize("name", ["two", "mixed", "prob", "modeb", "t64"])
def test_enough_workers_is_the_plain_walk(name):
    c = case(name)
    n = 600
    inv = invocations(name, BEGIN, n)
    per_service = np.bincount([x[0] for t in inv for x in t], minlength=len(c.sg.g.services))
    spans = reference(name, [max(1, int(k)) for k in per_service], n=n)
    assert np.array_equal(spans["start_ns"], spans["arrival_ns"])
    orec, _ = oc.run(c.sg, c.op, c.sg.entry(), BEGIN, n)
    assert np.array_equal(ref.latencies(spans), orec[:, 0])


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_the_gpu_cases_are_contended(name):
    """Non-vacuity, on the reference alone: with the workers the GPU tests give it, some invocation of a pooled
    service waits, and some start differs from the one-worker batch's."""
    c = case(name)
    workers = GRAPHS[name][5] if name not in ("two", "two_reps") else 2
    wl = np.array(worker_list(c, workers))
    arr = paced_arrivals(GRAPHS[name][3], GRAPHS[name][4]) if name == "ties_paced" else None
    pooled, single = reference(name, workers, arr=arr), reference(name, 1, arr=arr)
    waits = pooled["start_ns"] > pooled["arrival_ns"]
    assert np.any(waits & (wl[pooled["service"]] > 1))
    assert np.any(pooled["start_ns"] != single["start_ns"])


def test_the_tile_boundary_cases_wait_until_the_pool_is_the_batch():
    """`two` at its gap: every pool below the batch's 3,000 requests leaves somebody waiting, 4,096 nobody."""
    for W in (1, 2, 3, 63, 64, 65, 511, 513):
        s = reference("two", W)
        b = s[s["service"] == 1]
        assert len(b) == 3000 and np.any(b["start_ns"] > b["arrival_ns"]), W
    s = reference("two", 4096)
    assert np.array_equal(s["start_ns"], s["arrival_ns"])


def test_ties_graphs_have_equal_arrivals_in_one_replica():
    for name, arr in (("ties_paced", paced_arrivals(200_000, 2000)), ("ties_fanout", None)):
        s = reference(name, GRAPHS[name][5], arr=arr)
        ties = sum(int((np.diff(q["arrival_ns"].astype(np.int64)) == 0).sum()) for q in _by_replica(s)
                   if int(q["service"][0]) != 0 or name == "ties_fanout")
        assert ties > 100, (name, ties)


# ---- the class layout of csrc/des_workers.h

@pytest.mark.parametrize("W", [1, 2, 3, 7, 64, 65536])
def test_class_layout_is_a_permutation_with_contiguous_classes(W):
    for L in (1, 2, 3, 6, 7, 8, 63, 64, 65, 1000):
        p = np.arange(L)
        c, base, rem = p % W, L // W, L % W
        cs = c * base + np.minimum(c, rem)
        dst = cs + p // W
        assert sorted(dst.tolist()) == list(range(L))
        inv = np.argsort(dst)
        # along the new order: classes in turn, each in rank order, each keyed by its first index
        assert np.all(np.diff(c[inv]) >= 0)
        for k in np.unique(c):
            assert np.all(np.diff(p[inv][c[inv] == k]) == W) and len(set(cs[c == k])) == 1
        assert len(np.unique(cs)) == min(W, L)
