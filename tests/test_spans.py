"""Trace spans on the CPU: isim_trace_spans_host against the
Python oracle's event log and against the walk's records, the start times
against a hand-derived fixture and the rule's invariants, isim_select_traces_host
against numpy, and every argument the entry points refuse (all on the host,
before any HIP call)."""
import ctypes as C
import glob
import json
import os

import numpy as np
import pytest

import isim
from isim import native
from isim.yamljson import obj_to_json, yaml_to_json
from oracle import executor as oc
from oracle import graph_ref as gr
from oracle.executor_py import SimGraph, SimParams as OParams, run as py_run

import random_walk_graphs as rwg
from conftest import ROOT

N_TRACES = 200
NONE = 0xFFFFFFFF
TOPOLOGIES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "topologies", "*.yaml")))
# a dozen seeds of the dynamic family whose walk has an unrolled tree (a single sleep of 2^32 ns or more has none)
SEEDS = [s for s in rwg.SEEDS if not rwg.sleep_past_u32(rwg.dynamic_graph(s))][:12]
GRAPHS = [("topo:" + os.path.basename(p)[:-5], p) for p in TOPOLOGIES] + [(f"seed:{s}", s) for s in SEEDS]


def graph_of(src):
    """(graph JSON, SimParams for mode, first trace id) of a topology file or a random-graph seed."""
    if isinstance(src, str):
        return yaml_to_json(open(src, "rb").read()), lambda mode: isim.SimParams(error_mode=mode), (1 << 32) - 120
    return obj_to_json(rwg.dynamic_graph(src)), lambda mode: rwg.params(src, mode), (1 << 32) - 150 + 7 * src


def handler_of(j, p):
    p.flags |= native.FLAG_DYNAMIC
    return isim.Handler(isim.ServiceGraph.from_json(j), None, p)


def oracle_invocations(sg, op, begin, n):
    """Per trace the executed invocations (service, T, status, caller hop) in hop order, from the event log:
    a recv opens an invocation under the innermost open one, a resp closes it."""
    _, st = py_run(sg, op, sg.entry(), begin, n, events=True)
    traces, cur, stack = [], [], []
    for ev in st.events:
        if ev[0] == "recv":
            cur.append([ev[1], None, None, stack[-1] if stack else NONE])
            stack.append(len(cur) - 1)
        elif ev[0] == "resp":
            inv = cur[stack.pop()]
            assert inv[0] == ev[1]
            inv[1], inv[2] = ev[2], ev[3]
            if not stack:
                traces.append(cur)
                cur = []
    assert len(traces) == n and not cur
    return traces


def script_shape(doc):
    """Per service: the (step index, concurrent) of each call command in call-index order; and the first
    call-site id of each service (sites are numbered in document order)."""
    calls, base, nxt = [], [], 0
    for svc in doc["services"]:
        mine = []
        for si, step in enumerate(svc.get("script") or []):
            members = step if isinstance(step, list) else [step]
            mine += [(si, isinstance(step, list)) for m in members if "call" in m]
        calls.append(mine)
        base.append(nxt)
        nxt += len(mine)
    return calls, base


@pytest.fixture(scope="module", params=GRAPHS, ids=[g[0] for g in GRAPHS])
def walked(request):
    """One graph in both modes: the handler, the host spans of N_TRACES ids on both sides of 2^32, the oracle's
    invocations and records.  Computed once per graph, read by every test below."""
    j, params, begin = graph_of(request.param[1])
    doc = json.loads(j)
    out = []
    for mode in (isim.MODE_A, isim.MODE_B):
        p = params(mode)
        h = handler_of(j, p)
        ts = isim.TraceSpans(h)
        ids = np.arange(begin, begin + N_TRACES, dtype=np.uint64)
        off, spans, info = ts.raw_host(ids)
        sg = SimGraph(gr.unmarshal_service_graph(j))
        op = OParams(p.seed, p.hop_base_ns, p.req_ps_per_byte, p.resp_ps_per_byte, p.error_mode)
        orec, _ = oc.run(sg, op, sg.entry(), begin, N_TRACES, records=True)
        out.append(dict(mode=mode, h=h, off=off, spans=spans, info=info, sg=sg, op=op, begin=begin, orec=orec))
    return doc, out


def test_spans_equal_the_oracle_event_log(walked):
    _, runs = walked
    for r in runs:
        inv = oracle_invocations(r["sg"], r["op"], r["begin"], N_TRACES)
        off, s = r["off"], r["spans"]
        assert int(r["info"][native.SPAN_WRITTEN]) == N_TRACES and int(r["info"][native.SPAN_TOTAL]) == int(off[-1])
        for t in range(N_TRACES):
            sp = s[int(off[t]):int(off[t + 1])]
            assert len(sp) == len(inv[t])
            want = np.array(inv[t], dtype=np.uint64)
            assert np.array_equal(sp["hop"], np.arange(len(sp)))
            assert np.array_equal(sp["service"], want[:, 0])
            assert np.array_equal(sp["duration_ns"], want[:, 1])
            assert np.array_equal(sp["status"] & 1, want[:, 2])
            assert np.array_equal(sp["caller_hop"], want[:, 3])


def test_spans_equal_the_records(walked):
    _, runs = walked
    for r in runs:
        off, s, orec = r["off"], r["spans"], r["orec"]
        hops = (orec[:, 1] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        status_err = (orec[:, 1] >> np.uint64(32)).astype(np.uint64)
        assert np.array_equal(np.diff(off.astype(np.int64)), hops)
        first = off[:-1].astype(np.int64)
        assert np.array_equal(s["duration_ns"][first], orec[:, 0])
        assert np.array_equal(s["status"][first] & 1, status_err >> np.uint64(31))
        n500 = np.add.reduceat((s["status"] & 1).astype(np.int64), first)
        assert np.array_equal(n500, (status_err & np.uint64(0x7FFFFFFF)).astype(np.int64))
        # the own draw alone never makes a 200, and mode A has no failed steps
        assert not np.any((s["status"] & 3) == 2)
        if r["mode"] == isim.MODE_A:
            assert not np.any((s["status"] & 3) == 1)


def test_start_time_invariants(walked):
    doc, runs = walked
    calls, base = script_shape(doc)
    for r in runs:
        off, s, h = r["off"], r["spans"], r["h"]
        end = s["start_ns"] + s["hop_ns"] + s["duration_ns"]
        for t in range(N_TRACES):
            a, b = int(off[t]), int(off[t + 1])
            assert s["start_ns"][a] == 0
            step_of, step_start, before = {}, {}, {}   # per caller: current step, its start, end of earlier steps
            for i in range(a + 1, b):
                c = a + int(s["caller_hop"][i])
                svc = int(s["service"][c])
                k = int(h.slot_site[int(s["slot"][i])]) - base[svc]
                step, conc = calls[svc][k]
                start = int(s["start_ns"][i])
                # inside the caller
                assert int(end[i]) <= int(s["start_ns"][c]) + int(s["duration_ns"][c])
                if step_of.get(c) != step:
                    before[c] = max(before.get(c, 0), step_of.get((c, "end"), 0))
                    step_of[c], step_start[c], step_of[(c, "end")] = step, start, 0
                    assert start >= int(s["start_ns"][c])
                # sequential children do not overlap; the children of one concurrent step share a start
                assert start >= before[c]
                if conc:
                    assert start == step_start[c]
                step_of[(c, "end")] = max(step_of[(c, "end")], int(end[i]))


KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "spans_kat.json")))


@pytest.mark.parametrize("case", KAT["cases"], ids=[c["name"] for c in KAT["cases"]])
def test_start_times_known_answers(case):
    p = isim.SimParams(error_mode=case["mode"], **KAT["params"])
    h = handler_of(obj_to_json({"services": case["services"]}), p)
    tr = isim.TraceSpans(h).spans_host([7])[0]
    names = [s["name"] for s in case["services"]]
    assert len(tr) == len(case["spans"])
    for got, want in zip(tr.spans, case["spans"]):
        assert int(got["hop"]) == want["hop"] and int(got["caller_hop"]) == want["caller_hop"] & NONE
        assert names[int(got["service"])] == want["service"]
        for f in ("start_ns", "duration_ns", "hop_ns", "status"):
            assert int(got[f]) == want[f], (case["name"], want["hop"], f)
    text = tr.to_text().splitlines()
    assert len(text) == 1 + len(tr) and text[1].startswith(names[0] + " ")


def test_list_order_repeats_and_cap():
    j, params, _ = graph_of(SEEDS[1])
    ts = isim.TraceSpans(handler_of(j, params(isim.MODE_B)))
    ids = np.array([5, (1 << 63) + 1, 5, 0, (1 << 32) - 1, 1 << 32, 5], dtype=np.uint64)
    off, spans, info = ts.raw_host(ids)
    single = {int(i): ts.raw_host([i])[1] for i in set(ids.tolist())}
    for n, i in enumerate(ids.tolist()):
        assert np.array_equal(spans[int(off[n]):int(off[n + 1])], single[i])
    total = int(off[-1])
    # one span short: the last trace does not fit, the others are written, info says so
    off2, spans2, info2 = ts.raw_host(ids, cap_spans=total - 1)
    assert np.array_equal(off2, off) and list(info2) == [total, len(ids) - 1, len(ids), len(ids) - 1]
    assert np.array_equal(spans2[:int(off[-2])], spans[:int(off[-2])])
    assert not spans2[int(off[-2]):].view(np.uint8).any()
    off0, _, info0 = ts.raw_host([])
    assert list(off0) == [0] and list(info0) == [0, 0, 0, 0]


def test_select_host_against_numpy():
    rng = np.random.default_rng(11)
    n = 5000
    recs = np.zeros(n, isim.REC_DTYPE)
    recs["latency_ns"] = rng.integers(0, 1000, n, dtype=np.uint64)
    recs["latency_ns"][rng.random(n) < 0.01] = (1 << 64) - 1
    recs["status_err"] = np.where(rng.random(n) < 0.3, 0x80000003, 2).astype(np.uint32)
    begin = (1 << 32) - 100
    for thr in (0, 500, 990, 1000, (1 << 64) - 1):
        for cls in (native.Q_ALL, native.Q_200, native.Q_500):
            m = recs["latency_ns"] >= np.uint64(thr)
            if cls != native.Q_ALL:
                m &= (recs["status_err"] >> 31) == (1 if cls == native.Q_500 else 0)
            want = np.flatnonzero(m).astype(np.uint64) + np.uint64(begin)
            ids, matches = isim.select_traces_host(recs, begin, thr, cls)
            assert matches == len(want) and np.array_equal(ids, want)
            for cut in (0, 1, len(want), len(want) + 5):
                ids, matches = isim.select_traces_host(recs, begin, thr, cls, max_ids=cut)
                assert matches == len(want) and np.array_equal(ids, want[:cut])
    ids, matches = isim.select_traces_host(recs[:0], 0, 0)
    assert matches == 0 and len(ids) == 0


def _einval(fn, *args, match):
    rc = fn(*args)
    assert rc == native.EINVAL and match in native.last_error(), native.last_error()


def test_refusals_need_no_gpu():
    lib = native.load()
    topo = os.path.join(ROOT, "tests", "golden", "topologies", "canonical.yaml")
    j = yaml_to_json(open(topo, "rb").read())
    static = isim.Handler(isim.ServiceGraph.from_json(j), None, isim.SimParams())
    dag = isim.Handler(isim.ServiceGraph.from_json(j), None,
                       isim.SimParams(flags=native.FLAG_DYNAMIC | native.FLAG_TREE_DAG))
    good = handler_of(j, isim.SimParams())
    b = C.c_uint64()
    ids, off, info = np.zeros(4, np.uint64), np.zeros(5, np.uint64), np.zeros(4, np.uint64)
    spans = np.zeros(64, isim.SPAN_DTYPE)
    dev = (ids.ctypes.data, 4, off.ctypes.data, spans.ctypes.data, 64, info.ctypes.data)   # never dereferenced
    for h, why in ((static, "ISIM_FLAG_DYNAMIC"), (dag, "site graph")):
        _einval(lib.isim_trace_spans_workspace_bytes, h._h, 4, C.byref(b), match=why)
        _einval(lib.isim_trace_spans_host, h._h, *dev, match=why)
        _einval(lib.isim_trace_spans_device, h._h, *dev, None, 0, None, match=why)
        _einval(lib.isim_trace_spans, 0, h._h, *dev, match=why)
        with pytest.raises(isim.IsimError):
            isim.TraceSpans(h)
    native.check(lib.isim_trace_spans_workspace_bytes(good._h, 4, C.byref(b)))
    assert b.value > 0
    ws = np.zeros(b.value // 8 + 1, np.uint64)
    _einval(lib.isim_trace_spans_device, good._h, *dev, ws.ctypes.data, b.value - 1, None, match="workspace")
    _einval(lib.isim_trace_spans_device, good._h, *dev, None, b.value, None, match="workspace")
    _einval(lib.isim_trace_spans_workspace_bytes, good._h, (1 << 32) + 1, C.byref(b), match="2^32")
    _einval(lib.isim_trace_spans_device, good._h, ids.ctypes.data, (1 << 32) + 1, *dev[2:], ws.ctypes.data, 1 << 40,
            None, match="2^32")
    _einval(lib.isim_trace_spans_host, good._h, ids.ctypes.data, (1 << 32) + 1, *dev[2:], match="2^32")
    _einval(lib.isim_trace_spans_device, good._h, ids.ctypes.data + 4, *dev[1:], ws.ctypes.data, b.value, None,
            match="aligned")
    # the selection
    recs = np.zeros(4, isim.REC_DTYPE)
    _einval(lib.isim_select_traces_host, recs.ctypes.data, 4, 0, 0, 3, 4, ids.ctypes.data, info.ctypes.data,
            match="class")
    _einval(lib.isim_select_traces_device, recs.ctypes.data, 4, 0, 0, 0, 4, ids.ctypes.data, info.ctypes.data, None, 0,
            None, match="workspace")
    _einval(lib.isim_select_traces_device, recs.ctypes.data, (1 << 40) + 1, 0, 0, 0, 4, ids.ctypes.data,
            info.ctypes.data, ws.ctypes.data, 1 << 40, None, match="2^40")
    # a place call on spans that are not a walk's is refused, not followed
    bad = np.zeros(2, isim.SPAN_DTYPE)
    bad["caller_hop"] = 7
    _einval(lib.isim_trace_spans_place, good._h, np.array([0, 2], np.uint64).ctypes.data, 1, bad.ctypes.data,
            match="not those of a walk")
