"""Critical path on the CPU: isim_critical_path_host against a
plain Python restatement of the rule (recursive over the scripts and the host
spans, with start times of its own), bit for bit in start_ns, status and every
table word; the identity against the oracle's records, the invariants, the
corners of the winner rule (each asserted to occur), a hand-derived fixture,
merge, half lists, every refusal and the corrupted spans, all without a GPU."""
import ctypes as C
import glob
import json
import os
import re

import numpy as np
import pytest

import isim
from isim import native
from isim.yamljson import obj_to_json, yaml_to_json
from oracle import executor as oc
from oracle import graph_ref as gr
from oracle.executor_py import SimGraph, SimParams as OParams

import critical_path_graphs as cg
import random_walk_graphs as rwg
from conftest import ROOT

N_TRACES = 200
NONE = 0xFFFFFFFF
CRIT = native.SPAN_CRITICAL
ROW = native.CP_ROW_WORDS
M64 = (1 << 64) - 1
TOPOLOGIES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "topologies", "*.yaml")))
SEEDS = [s for s in rwg.SEEDS if not rwg.sleep_past_u32(rwg.dynamic_graph(s))][:12]
FREE = dict(hop_base_ns=0, req_ps_per_byte=0, resp_ps_per_byte=0)     # hops that cost nothing: children of cost 0
# (id, graph JSON, SimParams of a mode, first trace id): ids on both sides of 2^32 everywhere
GRAPHS = [("topo:" + os.path.basename(p)[:-5], yaml_to_json(open(p, "rb").read()),
           lambda mode: isim.SimParams(error_mode=mode, flags=native.FLAG_DYNAMIC), (1 << 32) - 120) for p in TOPOLOGIES]
GRAPHS += [(f"seed:{s}", obj_to_json(rwg.dynamic_graph(s)),
            (lambda s: lambda mode: _with(rwg.params(s, mode), native.FLAG_DYNAMIC))(s), (1 << 32) - 150 + 7 * s)
           for s in SEEDS]
GRAPHS += [(f"hand:{name}", obj_to_json(cg.CASES[name][0]),
            (lambda fl: lambda mode: isim.SimParams(error_mode=mode, flags=fl))(cg.CASES[name][1]), (1 << 32) - 100)
           for name in cg.CASES]
GRAPHS += [("hand:winners-free-hops", obj_to_json(cg.winners()),
            lambda mode: isim.SimParams(error_mode=mode, flags=cg.D, **FREE), (1 << 32) - 100),
           # the widest random graph once more on the 16-byte nodes
           ("seed-wide:%d" % SEEDS[3], obj_to_json(rwg.dynamic_graph(SEEDS[3])),
            lambda mode: _with(rwg.params(SEEDS[3], mode), cg.D | cg.W), (1 << 32) - 90)]


def _with(p, flags):
    p.flags |= flags
    return p


def restate(scripts, call_index, sp, cover):
    """The rule, recursively from the entry: (start_ns, critical, self_ns) per hop of one trace's spans.
    scripts: per service the canonical script; call_index(i): the call command of span i in its caller."""
    m = len(sp)
    kids = [[] for _ in range(m)]
    for i in range(1, m):
        kids[int(sp["caller_hop"][i])].append(i)
    start, critical, self_ns = [0] * m, [False] * m, [0] * m
    cost = [int(sp["hop_ns"][i]) + int(sp["duration_ns"][i]) for i in range(m)]

    def visit(i, at, crit):
        start[i], critical[i] = at, crit
        mine, nxt, k, clock, won = kids[i], 0, 0, at, 0

        def take():
            nonlocal nxt, k
            k += 1
            if nxt < len(mine) and call_index(mine[nxt]) == k - 1:
                nxt += 1
                return mine[nxt - 1]
            return None

        for cmd in scripts[int(sp["service"][i])]:
            if nxt == len(mine):
                break           # every executed child is placed: only the caller's own time is left
            if cmd[0] == "sleep":
                clock += max(cmd[1], 0)
            elif cmd[0] == "call":
                c = take()
                if c is not None:
                    visit(c, clock, crit)
                    won += cost[c]
                    clock += cost[c]
            else:
                longest, winner, members = 0, None, []
                for x in cmd[1]:
                    c = take() if x[0] == "call" else None
                    val = cost[c] if c is not None else (max(x[1], 0) if x[0] == "sleep" else 0)
                    who = c if x[0] == "call" else "sleep"
                    members.append((x[0], c, val))
                    if val > longest:
                        longest, winner = val, who
                    elif val == longest and val > 0 and c is not None and winner not in (None, "sleep"):
                        cover["tie"] += 1
                for _, c, _ in members:
                    if c is not None:
                        visit(c, clock, crit and c == winner)
                calls = [(c, val) for kind, c, val in members if kind == "call"]
                cover["sleep_won"] += winner == "sleep"
                cover["no_winner"] += winner is None
                cover["zero_cost_child"] += any(c is not None and val == 0 for c, val in calls)
                cover["first_skipped_later_wins"] += bool(calls) and calls[0][0] is None and winner not in (None, "sleep")
                if winner not in (None, "sleep"):
                    won += longest
                clock += longest
        self_ns[i] = int(sp["duration_ns"][i]) - won

    visit(0, 0, True)
    return start, critical, self_ns


def restated_table(n_services, sp, critical, self_ns):
    t = np.zeros((n_services + 1, ROW), dtype=object)
    for i in range(len(sp)):
        r = t[int(sp["service"][i])]
        r[native.CP_INVOCATIONS] += 1
        r[native.CP_SUM_DURATION] += int(sp["duration_ns"][i])
        if critical[i]:
            r[native.CP_CRITICAL] += 1
            r[native.CP_SELF_NS] += self_ns[i]
            r[native.CP_HOP_NS] += int(sp["hop_ns"][i])
            r[native.CP_CRITICAL_500] += int(sp["status"][i]) & 1
    h = t[n_services]
    h[native.CP_H_TRACES] += 1
    h[native.CP_H_SPANS] += len(sp)
    h[native.CP_H_CRITICAL] += sum(critical)
    h[native.CP_H_SUM_LATENCY] += int(sp["duration_ns"][0])
    return t


def call_bases(scripts):
    """The first call-site id of each service (sites are numbered in document order)."""
    base, nxt = [], 0
    for sc in scripts:
        base.append(nxt)
        nxt += sum(1 for cmd in sc for x in (cmd[1] if cmd[0] == "conc" else [cmd]) if x[0] == "call")
    return base


CORNERS = ("tie", "sleep_won", "no_winner", "zero_cost_child", "first_skipped_later_wins", "mode_b_failed_step")
COVER = {}      # graph index -> how often its traces met each corner


def fold_graph(idx):
    """One graph in both modes: the host spans of N_TRACES ids with their start times zeroed (what the
    device call gets), folded by isim_critical_path_host; the restatement; the oracle's records."""
    _, j, params, begin = GRAPHS[idx]
    out = []
    cover = COVER[idx] = dict.fromkeys(CORNERS, 0)
    for mode in (isim.MODE_A, isim.MODE_B):
        p = params(mode)
        h = isim.Handler(isim.ServiceGraph.from_json(j), None, p)
        ts = isim.TraceSpans(h)
        scripts = [s["script"] for s in h.graph.canonical()["services"]]
        base = call_bases(scripts)
        ids = np.arange(begin, begin + N_TRACES, dtype=np.uint64)
        off, placed, info = ts.raw_host(ids)
        assert int(info[native.SPAN_WRITTEN]) == N_TRACES
        spans = placed.copy()
        spans["start_ns"] = 0
        table = ts.fold_host(off, spans, N_TRACES)
        want = np.zeros((len(scripts) + 1, ROW), dtype=object)
        per_trace = []
        for t in range(N_TRACES):
            sp = placed[int(off[t]):int(off[t + 1])]

            def call_index(i, sp=sp):
                svc = int(sp["service"][int(sp["caller_hop"][i])])
                return int(h.slot_site[int(sp["slot"][i])]) - base[svc]

            st, cr, se = restate(scripts, call_index, sp, cover)
            per_trace.append((st, cr, se))
            want += restated_table(len(scripts), sp, cr, se)
        cover["mode_b_failed_step"] += int(np.count_nonzero((placed["status"] & 3) == 1))
        sg = SimGraph(gr.unmarshal_service_graph(j))
        op = OParams(p.seed, p.hop_base_ns, p.req_ps_per_byte, p.resp_ps_per_byte, p.error_mode)
        orec, _ = oc.run(sg, op, sg.entry(), begin, N_TRACES, records=True)
        out.append(dict(mode=mode, h=h, ts=ts, off=off, placed=placed, spans=spans, table=table, want=want,
                        per_trace=per_trace, orec=orec, n_services=len(scripts)))
    return out


@pytest.fixture(scope="module", params=range(len(GRAPHS)), ids=[g[0] for g in GRAPHS])
def folded(request):
    """Computed once per graph, read by every test below."""
    return fold_graph(request.param)


def test_host_equals_the_restatement(folded):
    for r in folded:
        off, s, placed = r["off"], r["spans"], r["placed"]
        for t, (st, cr, _) in enumerate(r["per_trace"]):
            a, b = int(off[t]), int(off[t + 1])
            assert s["start_ns"][a:b].tolist() == st, t
            assert (s["status"][a:b] ^ placed["status"][a:b]).tolist() == [CRIT if c else 0 for c in cr], t
        # nothing but start_ns and the bit changed
        back = s.copy()
        back["status"] &= ~np.uint32(CRIT)
        back["start_ns"] = placed["start_ns"]
        assert back.tobytes() == placed.tobytes()
        assert r["table"].tolist() == [int(x) & M64 for x in r["want"].reshape(-1)]
        assert all(se >= 0 for _, _, ses in r["per_trace"] for se in ses)


def test_reproduces_the_placed_start_times(folded):
    for r in folded:
        # the start times of isim_trace_spans_place, from zeroed ones and again over the placed spans
        assert np.array_equal(r["spans"]["start_ns"], r["placed"]["start_ns"])
        again = r["placed"].copy()
        r["ts"].place(r["off"], again, N_TRACES)
        table = r["ts"].fold_host(r["off"], again, N_TRACES)
        assert again.tobytes() == r["spans"].tobytes() and np.array_equal(table, r["table"])


def test_identity_and_invariants(folded):
    for r in folded:
        off, s, n_s = r["off"], r["spans"], r["n_services"]
        table = r["table"].reshape(n_s + 1, ROW)
        for t, (_, cr, se) in enumerate(r["per_trace"]):
            a, b = int(off[t]), int(off[t + 1])
            sp = s[a:b]
            crit = (sp["status"] & CRIT) != 0
            # the parts sum to the record's latency exactly
            assert sum(se[i] + int(sp["hop_ns"][i]) for i in np.flatnonzero(crit)) == int(r["orec"][t, 0])
            # one subtree that holds the entry: every critical span but the entry has a critical caller
            assert crit[0] and all(crit[int(sp["caller_hop"][i])] for i in np.flatnonzero(crit)[1:])
        rows, hdr = table[:-1].astype(object), table[-1]
        assert (rows[:, native.CP_SELF_NS].sum() + rows[:, native.CP_HOP_NS].sum()) & M64 == int(hdr[native.CP_H_SUM_LATENCY])
        assert int(hdr[native.CP_H_SUM_LATENCY]) == int(r["orec"][:, 0].astype(object).sum()) & M64
        assert np.all(table[:-1, native.CP_CRITICAL] <= table[:-1, native.CP_INVOCATIONS])
        assert np.all(table[:-1, native.CP_CRITICAL_500] <= table[:-1, native.CP_CRITICAL])
        assert hdr.tolist() == [N_TRACES, int(off[-1]), int(table[:-1, native.CP_CRITICAL].sum()),
                                int(hdr[native.CP_H_SUM_LATENCY]), 0, 0]
        assert int(table[:-1, native.CP_INVOCATIONS].sum()) == int(off[-1])


def test_halves_merge_to_the_whole(folded):
    r = folded[1]
    ts, off, n_s = r["ts"], r["off"], r["n_services"]
    half = N_TRACES // 2
    a = r["placed"][:int(off[half])].copy()
    b = r["placed"][int(off[half]):].copy()
    off_a = off[:half + 1].copy()
    off_b = (off[half:] - off[half]).copy()
    cp_a = isim.CriticalPath(r["h"], ts.fold_host(off_a, a, half), ts.names)
    cp_b = isim.CriticalPath(r["h"], ts.fold_host(off_b, b, N_TRACES - half), ts.names)
    before = cp_a.table.astype(object) + cp_b.table.astype(object)
    cp_a.merge(cp_b)                                        # merge is addition
    assert cp_a.table.reshape(-1).tolist() == [int(x) & M64 for x in before.reshape(-1)]
    assert np.array_equal(cp_a.table.reshape(-1), r["table"])
    assert np.concatenate([a, b]).tobytes() == r["spans"].tobytes()
    # and a table that starts non-zero takes the adds on top (mod 2^64)
    start = np.full(r["table"].shape, M64 - 5, np.uint64)
    got = ts.fold_host(off, r["placed"].copy(), N_TRACES, start.copy())
    assert got.tolist() == [(int(x) + M64 - 5) & M64 for x in r["table"]]
    assert n_s + 1 == cp_a.table.shape[0] and ts.table_words() == (n_s + 1) * ROW


def test_the_corners_of_the_rule_occurred():
    """Across the graphs above each corner of the rule is met (a graph the tests above have not folded in
    this run is folded here)."""
    for idx in range(len(GRAPHS)):
        if idx not in COVER:
            fold_graph(idx)
    for corner in CORNERS:
        assert sum(c[corner] for c in COVER.values()) > 0, corner


KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "critical_path_kat.json")))


@pytest.mark.parametrize("case", KAT["cases"], ids=[c["name"] for c in KAT["cases"]])
def test_known_answers(case):
    p = isim.SimParams(error_mode=case["mode"], flags=native.FLAG_DYNAMIC, **KAT["params"])
    h = isim.Handler(isim.ServiceGraph.from_json(obj_to_json({"services": case["services"]})), None, p)
    cp = isim.TraceSpans(h).critical_path_host([7])
    names = [s["name"] for s in case["services"]]
    tr = cp.traces[0]
    assert len(tr) == len(case["spans"]) and len(names) <= 6
    crit = set(tr.critical().tolist())
    assert crit == {w["hop"] for w in case["spans"] if w["critical"]}
    for got, want in zip(tr.spans, case["spans"]):
        assert names[int(got["service"])] == want["service"] and int(got["start_ns"]) == want["start_ns"]
        if want["critical"]:    # the self time from the marked spans: the duration less its critical children
            mine = [c for c in crit if int(tr.spans["caller_hop"][c]) == want["hop"]]
            self_ns = int(got["duration_ns"]) - sum(int(tr.spans["hop_ns"][c]) + int(tr.spans["duration_ns"][c])
                                                    for c in mine)
            assert self_ns == want["self_ns"], want
    want_table = [case["table"][n] for n in names] + [case["table"]["header"]]
    assert cp.table.tolist() == want_table
    rows = cp.rows()
    assert [r["path_ns"] for r in rows] == sorted((r["path_ns"] for r in rows), reverse=True)
    assert sum(r["path_ns"] for r in rows) == cp.header["sum_latency_ns"] == tr.latency_ns
    assert abs(sum(r["share"] for r in rows) - 1) < 1e-9
    text = tr.to_text().splitlines()
    assert [l.endswith(" *") for l in text[1:]] == [w["critical"] for w in case["spans"]]
    assert cp.to_text().splitlines()[2].startswith(rows[0]["service"])


def test_a_trace_without_the_bit_prints_as_before():
    h = cg.make("winners", isim.MODE_A)
    ts = isim.TraceSpans(h)
    plain, marked = ts.spans_host([3])[0], ts.critical_path_host([3]).traces[0]
    assert " *" not in plain.to_text()
    assert marked.to_text().replace(" *", "") == plain.to_text() and " *" in marked.to_text()


def _einval(fn, *args, match):
    rc = fn(*args)
    assert rc == native.EINVAL and match in native.last_error(), native.last_error()


def test_refusals_need_no_gpu():
    lib = native.load()
    j = yaml_to_json(open(os.path.join(ROOT, "tests", "golden", "topologies", "canonical.yaml"), "rb").read())
    static = isim.Handler(isim.ServiceGraph.from_json(j), None, isim.SimParams())
    dag = isim.Handler(isim.ServiceGraph.from_json(j), None,
                       isim.SimParams(flags=native.FLAG_DYNAMIC | native.FLAG_TREE_DAG))
    good = isim.Handler(isim.ServiceGraph.from_json(j), None, isim.SimParams(flags=native.FLAG_DYNAMIC))
    ts = isim.TraceSpans(good)
    off, spans, _ = ts.raw_host([1, 2])
    cap = len(spans)
    table, info = np.zeros(ts.table_words(), np.uint64), np.array([cap, 2, 2, 2], np.uint64)
    b = C.c_uint64()
    native.check(lib.isim_critical_path_workspace_bytes(good._h, cap, C.byref(b)))
    assert 0 < b.value <= 8 * cap + 64                    # at most 8 bytes per span plus a constant
    ws = np.zeros(b.value // 8 + 1, np.uint64)
    # (host arrays stand in for device buffers: every call below returns before it would touch them)
    dev = [off.ctypes.data, spans.ctypes.data, cap, info.ctypes.data, 2, table.ctypes.data, ws.ctypes.data, b.value, None]
    for h, why in ((static, "ISIM_FLAG_DYNAMIC"), (dag, "site graph")):
        _einval(lib.isim_critical_path_table_words, h._h, C.byref(b), match=why)
        _einval(lib.isim_critical_path_workspace_bytes, h._h, cap, C.byref(b), match=why)
        _einval(lib.isim_critical_path_merge, h._h, table.ctypes.data, table.ctypes.data, match=why)
        _einval(lib.isim_critical_path_host, h._h, off.ctypes.data, 2, spans.ctypes.data, table.ctypes.data, match=why)
        _einval(lib.isim_critical_path_device, h._h, *dev, match=why)
        _einval(lib.isim_critical_path, 0, h._h, off.ctypes.data, 2, spans.ctypes.data, table.ctypes.data, match=why)
    _einval(lib.isim_critical_path_device, None, *dev, match="null handler")
    for i, why in ((0, "null"), (1, "null spans"), (3, "null"), (5, "null"), (6, "workspace")):
        bad = list(dev)
        bad[i] = None
        _einval(lib.isim_critical_path_device, good._h, *bad, match=why)
    for i in (0, 1, 3, 5, 6):
        bad = list(dev)
        bad[i] += 4
        _einval(lib.isim_critical_path_device, good._h, *bad, match="aligned")
    short = list(dev)
    short[7] -= 1
    _einval(lib.isim_critical_path_device, good._h, *short, match="workspace")
    many = list(dev)
    many[4] = (1 << 32) + 1
    _einval(lib.isim_critical_path_device, good._h, *many, match="2^32")
    _einval(lib.isim_critical_path_host, good._h, off.ctypes.data, (1 << 32) + 1, spans.ctypes.data, table.ctypes.data,
            match="2^32")
    _einval(lib.isim_critical_path_host, good._h, None, 2, spans.ctypes.data, table.ctypes.data, match="null")
    _einval(lib.isim_critical_path_host, good._h, off.ctypes.data, 2, spans.ctypes.data, None, match="null")
    _einval(lib.isim_critical_path_host, good._h, off.ctypes.data, 2, None, table.ctypes.data, match="null spans")
    _einval(lib.isim_critical_path_host, good._h, off.ctypes.data, 2, spans.ctypes.data + 4, table.ctypes.data,
            match="aligned")
    _einval(lib.isim_critical_path_merge, good._h, None, table.ctypes.data, match="null")
    _einval(lib.isim_critical_path_table_words, good._h, None, match="null")
    assert not table.any()
    # a self time below 0 (durations that are no walk's) is an error, not a wrapped sum
    forged = spans.copy()
    forged["duration_ns"][0] = 1
    assert len(forged) > off[1] > 1
    _einval(lib.isim_critical_path_host, good._h, off.ctypes.data, 2, forged.ctypes.data, table.ctypes.data,
            match="self time below 0")


@pytest.mark.parametrize("kind", cg.CORRUPTIONS)
def test_corrupted_spans_are_refused_and_counted(kind):
    h = cg.make("winners", isim.MODE_B)
    ts = isim.TraceSpans(h)
    n, n_s, victim = 40, len(ts.names), 17
    true_off, spans, _ = ts.raw_host(np.arange(100, 100 + n, dtype=np.uint64))
    spans["start_ns"] = 0
    off = true_off.copy()
    refused = cg.corrupt(kind, off, spans, victim, 0xFFFFFFF0, n_s)
    before = spans.copy()
    table = ts.fold_host(off, spans, n).reshape(n_s + 1, ROW)
    # the other traces alone, as a list of their own
    keep = [i for i in range(n) if i not in refused]
    sel = np.concatenate([np.arange(int(true_off[i]), int(true_off[i + 1])) for i in keep])
    others = before[sel].copy()
    others_off = np.concatenate([[0], np.cumsum([int(true_off[i + 1] - true_off[i]) for i in keep])]).astype(np.uint64)
    want = ts.fold_host(others_off, others, len(keep)).reshape(n_s + 1, ROW)
    want[-1, native.CP_H_REFUSED] = len(refused)
    assert int(table[-1, native.CP_H_TRACES]) == n - len(refused)
    assert np.array_equal(table, want)                              # refused, counted, the table otherwise unchanged
    assert spans[sel].tobytes() == others.tobytes()                 # the others as ever
    rest = np.setdiff1d(np.arange(len(spans)), sel)
    assert spans[rest].tobytes() == before[rest].tobytes()          # the refused traces untouched


def test_symbols_agree_across_header_python_and_go():
    hdr = open(os.path.join(ROOT, "include", "isim.h")).read()
    go = open(os.path.join(ROOT, "go", "isim", "isim.go")).read()
    fns = ("isim_critical_path_table_words", "isim_critical_path_workspace_bytes", "isim_critical_path_merge",
           "isim_critical_path_device", "isim_critical_path_host", "isim_critical_path")
    lib = native.load()
    for fn in fns:
        assert re.search(r"ISIM_API int %s\(" % fn, hdr) and fn in native.SIGNATURES and hasattr(lib, fn), fn
    assert "C.isim_critical_path(" in go and "C.isim_critical_path_table_words(" in go
    consts = dict(SPAN_CRITICAL=4, CP_INVOCATIONS=0, CP_SUM_DURATION=1, CP_CRITICAL=2, CP_SELF_NS=3, CP_HOP_NS=4,
                  CP_CRITICAL_500=5, CP_ROW_WORDS=6, CP_H_TRACES=0, CP_H_SPANS=1, CP_H_CRITICAL=2,
                  CP_H_SUM_LATENCY=3, CP_H_REFUSED=4)
    for name, val in consts.items():
        m = re.search(r"#define ISIM_%s\s+(\d+)u?\b" % name, hdr)
        assert m and int(m.group(1)) == val == getattr(native, name), name
        assert "C.ISIM_%s" % name in go, name
    assert re.search(r"#define ISIM_ABI_VERSION\s+10\b", hdr) and native.ABI_VERSION == 10
    assert lib.isim_abi_version() == 10
