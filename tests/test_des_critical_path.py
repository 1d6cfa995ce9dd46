"""DES critical path on the CPU: isim_des_critical_path_host
against the recursive Python restatement (tests/des_critical_path_ref.py) on
the spans of the pinned DES restatement (tests/des_spans_ref.py): every status
bit, table word and per-trace critical wait; the arrival equation on every
child; the identity against the C oracle; the contention-free limit against
isim_critical_path_host; a hand-written graph whose corners are counted;
hand-derived vectors; merge; every refusal; corrupted spans."""
import collections
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import isim
from isim import native
from isim.des_spans import des_critical_path_host
from oracle import des as od

import des_critical_path_ref as cref
import des_spans_ref as ref
from test_des_gpu import DesCase
from test_des_spans import ALL, BEGIN, N, _handlers, case_of, reference

NONE = 0xFFFFFFFF
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
MEANS = [300_000, 3_000_000]


def to_spans(rows):
    """REF_DTYPE rows as isim_des_span records (slot: the site, which no fold reads)."""
    out = np.zeros(len(rows), isim.DES_SPAN_DTYPE)
    for f in ("arrival_ns", "start_ns", "finish_ns", "hop_ns", "hop", "caller_hop", "position", "service", "status",
              "replica"):
        out[f] = rows[f]
    out["slot"] = rows["site"]
    return out


def offsets(rows):
    first = np.flatnonzero(rows["hop"] == 0)
    return np.concatenate([first, [len(rows)]]).astype(np.uint64)


def n_positions(sg):
    t = ref._Tree(sg)
    return t.subtree(sg.entry())


def host_fold(h, off, spans, table=None, n=None):
    n = len(off) - 1 if n is None else n
    s = spans.copy()
    words = (h.info.n_services + 1) * native.DCP_ROW_WORDS
    t = np.zeros(words, np.uint64) if table is None else table.copy().ravel()
    w = np.full(max(1, n), 0x1111, np.uint64)
    des_critical_path_host(h, np.ascontiguousarray(off, np.uint64), n, s, t, w)
    return s, t.reshape(-1, native.DCP_ROW_WORDS), w[:n]


def check_against_ref(c, rows):
    """The host fold of the whole batch equals the restatement; returns what both gave."""
    off, spans = offsets(rows), to_spans(rows)
    eqs = []
    bits, table, waits = cref.fold(c.sg, rows, off, n_positions(c.sg), equations=eqs)
    # the arrival equation on every child span (the rule matches §10.1)
    assert len(eqs) == int((rows["hop"] != 0).sum())
    idx, want = np.array([e[0] for e in eqs], np.int64), np.array([e[1] for e in eqs], np.uint64)
    assert np.array_equal(rows["arrival_ns"][idx], want)
    s, t, w = host_fold(c.h, off, spans)
    assert np.array_equal(s["status"], spans["status"] | bits)
    untouched = [f for f in spans.dtype.names if f != "status"]
    assert np.array_equal(s[untouched], spans[untouched])
    assert np.array_equal(t, table), (t, table)
    assert np.array_equal(w, waits)
    ns = c.h.info.n_services
    assert int(t[ns, native.DCP_H_REFUSED]) == 0 and int(t[ns, native.DCP_H_TRACES]) == len(off) - 1
    part = t[:ns, native.DCP_WAIT_NS] + t[:ns, native.DCP_SELF_NS] + t[:ns, native.DCP_HOP_NS]
    assert int(part.sum()) == int(t[ns, native.DCP_H_SUM_LATENCY])
    return off, s, t, w


@pytest.mark.parametrize("mean", MEANS)
@pytest.mark.parametrize("case", ALL, ids=[c[0] for c in ALL])
def test_host_fold_equals_the_restatement(case, mean):
    _, name, mode = case
    c = case_of(name, mode, mean)
    rows = reference(name, mode, mean)
    off, s, t, w = check_against_ref(c, rows)
    # the identity per trace, against the C DES oracle's latency_ns
    orec, _, _ = od.run(c.sg, c.op, c.sg.entry(), BEGIN, N, mean, og=c.og)
    crit = (s["status"] & native.SPAN_CRITICAL) != 0
    trace = np.repeat(np.arange(N), np.diff(off.astype(np.int64)))
    self_plus = np.zeros(N, np.uint64)
    # wait + hop of the critical spans, and self from the children that won: per trace the sum is the latency
    kids_won = np.zeros(len(s), np.uint64)
    child = np.flatnonzero(crit & (s["hop"] != 0))
    caller = off[trace[child]].astype(np.int64) + s["caller_hop"][child].astype(np.int64)
    np.add.at(kids_won, caller, s["hop_ns"][child] + s["finish_ns"][child] - s["arrival_ns"][child])
    parts = (s["finish_ns"] - s["arrival_ns"]) + s["hop_ns"] - kids_won   # wait + self + hop of a critical span
    np.add.at(self_plus, trace[crit], parts[crit])
    assert np.array_equal(self_plus, orec[:, 0])
    # the per-trace critical wait is the sum of S - a over the trace's critical spans
    crit_wait = np.zeros(N, np.uint64)
    np.add.at(crit_wait, trace[crit], (s["start_ns"] - s["arrival_ns"])[crit])
    assert np.array_equal(w, crit_wait)


@pytest.mark.parametrize("graph", [("canonical_p50", isim.MODE_A), ("seq_tree_abort", isim.MODE_B)],
                         ids=["canonical_p50", "seq_tree_abort"])
def test_trace_ids_on_both_sides_of_2_32(graph):
    begin, n = (1 << 32) - 300, 601
    c = case_of(*graph, 300_000)
    check_against_ref(c, reference(*graph, 300_000, begin, n))


# (graphs whose traces do not queue behind themselves: no service is reached twice at one instant of one trace)
@pytest.mark.parametrize("graph", [("seq_tree_p50", isim.MODE_A), ("canonical_p50", isim.MODE_A),
                                   ("seq_tree_abort", isim.MODE_B)], ids=["seq_tree_p50", "canonical_p50", "abort_b"])
def test_without_contention_it_is_the_walk_critical_path(graph):
    mean = 1 << 34      # the largest mean gap: 17 s between arrivals, nothing waits
    name, mode = graph
    c = case_of(name, mode, mean)
    n = 400
    rows = ref.simulate(c.sg, c.op, BEGIN, n, ref.arrivals(c.op.seed, mean, BEGIN, n))
    assert np.array_equal(rows["start_ns"], rows["arrival_ns"])
    off, s, t, w = check_against_ref(c, rows)
    ns = c.h.info.n_services
    assert not t[:ns, native.DCP_WAIT_NS].any() and not t[:ns, native.DCP_CRITICAL_WAITED].any() and not w.any()
    walk = isim.TraceSpans(c.h).critical_path_host(np.arange(BEGIN, BEGIN + n, dtype=np.uint64))
    ws = np.concatenate([tr.spans for tr in walk.traces])
    assert np.array_equal(ws["position"], s["position"]) and np.array_equal(ws["hop"], s["hop"])
    assert np.array_equal(ws["status"] & native.SPAN_CRITICAL, s["status"] & native.SPAN_CRITICAL)
    for dw, cw in ((native.DCP_CRITICAL, native.CP_CRITICAL), (native.DCP_SELF_NS, native.CP_SELF_NS),
                   (native.DCP_HOP_NS, native.CP_HOP_NS), (native.DCP_INVOCATIONS, native.CP_INVOCATIONS)):
        assert np.array_equal(t[:ns, dw], walk.table[:ns, cw])


def corner_doc(err=0.0):
    """e's concurrent steps: a (short script, one busy replica) against b (long script, many replicas); two
    calls that may both be skipped; a call that may be skipped before one that runs; a sleep against a short
    call; two equal callees."""
    return {"services": [
        {"name": "e", "isEntrypoint": True, "numReplicas": 64,
         "script": [[{"call": "a"}, {"call": "b"}],
                    [{"call": {"service": "c", "probability": 50}}, {"call": {"service": "c", "probability": 50}}],
                    [{"call": {"service": "c", "probability": 50}}, {"call": "d"}],
                    [{"sleep": "5ms"}, {"call": "f"}],
                    [{"call": "g"}, {"call": "g"}]]},
        {"name": "a", "script": [{"sleep": "1ms"}]},
        {"name": "b", "numReplicas": 64, "script": [{"sleep": "3ms"}]},
        {"name": "c", "numReplicas": 64, "script": [{"sleep": "200us"}]},
        {"name": "d", "numReplicas": 64, "errorRate": err, "script": [{"sleep": "100us"}]},
        {"name": "f", "numReplicas": 64, "script": [{"sleep": "1ms"}]},
        {"name": "g", "numReplicas": 64, "script": [{"sleep": "1ms"}]},
    ]}


@functools.lru_cache(maxsize=None)
def corner_run(mean, mode=isim.MODE_A, err=0.0, n=300):
    c = DesCase(corner_doc(err), mean, error_mode=mode, flags=native.FLAG_DYNAMIC)
    assert c.d.info.items == 1
    rows = ref.simulate(c.sg, c.op, 0, n, ref.arrivals(c.op.seed, mean, 0, n))
    return c, rows


def test_corners_of_a_hand_written_graph():
    c, rows = corner_run(300_000)
    off, s, t, w = check_against_ref(c, rows)
    corners = collections.Counter()
    cref.fold(c.sg, rows, off, n_positions(c.sg), corners=corners)
    for what in ("sleep_won", "tie", "no_winner", "skipped_then_later"):
        assert corners[what] > 0, (what, corners)
    crit = (s["status"] & native.SPAN_CRITICAL) != 0
    assert int((crit & (s["start_ns"] > s["arrival_ns"])).sum()) > 0      # a critical span that waited
    # the first step's winner under contention is a (behind its one busy replica); without contention it is b
    free_c, free_rows = corner_run(1 << 34)
    _, fs, _, _ = check_against_ref(free_c, free_rows)
    names = [x["name"] for x in c.h.graph.canonical()["services"]]
    a, b = names.index("a"), names.index("b")
    fcrit = (fs["status"] & native.SPAN_CRITICAL) != 0
    assert fcrit[fs["service"] == b].all() and not fcrit[fs["service"] == a].any()
    flipped = int(crit[s["service"] == a].sum())
    assert flipped > 0 and int(crit[s["service"] == a].sum()) + int(crit[s["service"] == b].sum()) == len(off) - 1
    assert int(t[a, native.DCP_WAIT_NS]) > 0 and int(t[a, native.DCP_CRITICAL_WAITED]) == flipped


def test_a_mode_b_failed_step():
    c, rows = corner_run(300_000, isim.MODE_B, 0.4)
    off, s, t, w = check_against_ref(c, rows)
    names = [x["name"] for x in c.h.graph.canonical()["services"]]
    d, f = names.index("d"), names.index("f")
    failed = 0
    for i in range(len(off) - 1):
        tr = s[int(off[i]):int(off[i + 1])]
        d500 = bool((tr["status"][tr["service"] == d] & 1).any())
        assert d500 != bool((tr["service"] == f).any())        # nothing follows the failed step
        failed += d500
    assert 0 < failed < len(off) - 1


KAT = os.path.join(os.path.dirname(__file__), "golden", "des_critical_path_kat.json")


def _kat():
    with open(KAT) as fh:
        k = json.load(fh)
    c = DesCase(k["graph"], 300_000, flags=native.FLAG_DYNAMIC)
    return k, c


def test_hand_derived_vectors():
    """Graph: e = sleep 1 ms, then {a | b} concurrently, then c; a sleeps 2 ms, b and c 1 ms; every hop 50 us.
    Spans are [arrival, start, finish, hop_ns, hop, caller, position, site, service, status]; times in ns.

    no_waits: e starts at 0; its clock is 1,000,000 at the step.  a and b arrive at 1,050,000; a runs 2 ms
      (value 50,000 + 2,000,000 = 2,050,000), b 1 ms (1,050,000): a wins, the clock is 3,050,000.  c arrives at
      3,100,000, runs 1 ms (value 1,050,000): e finishes at 4,100,000.  Critical: e, a, c.  self(e) = 4,100,000 -
      (2,050,000 + 1,050,000) = 1,000,000; a: self 2,000,000, hop 50,000; c: self 1,000,000, hop 50,000.
      1,000,000 + 2,050,000 + 1,050,000 = 4,100,000.
    the_queued_callee_wins: b waits until 3,000,000 (wait 1,950,000) and finishes at 4,000,000: its value is
      50,000 + 2,950,000 = 3,000,000 > a's 2,050,000, so b wins although its script is the shorter; the clock
      is 4,000,000.  c arrives at 4,050,000, waits 200,000, finishes at 5,250,000 (value 1,250,000) = e's
      finish.  Critical: e, b, c.  self(e) = 5,250,000 - 4,250,000 = 1,000,000; b: wait 1,950,000, self
      1,000,000, hop 50,000; c: wait 200,000, self 1,000,000, hop 50,000.  Sum 5,250,000; the trace's critical
      wait is 2,150,000.
    tie_entry_wait_and_a_500: e arrives at 1,000 and starts at 501,000 (wait 500,000); the clock is 1,501,000
      at the step.  a: arrives 1,551,000, finishes 3,551,000 with a 500 (value 2,050,000).  b: waits 1,000,000,
      finishes 3,551,000 (value 2,050,000): a tie, the first listed member a wins; b's wait is not on the path.
      Nothing follows (mode B's failed step): e finishes at 3,551,000, latency 3,550,000.  Critical: e, a.
      e: wait 500,000, self 3,050,000 - 2,050,000 = 1,000,000; a: self 2,000,000, hop 50,000.  Sum 3,550,000.
    """
    k, c = _kat()
    assert [x["name"] for x in c.h.graph.canonical()["services"]] == ["e", "a", "b", "c"]
    dt = np.dtype([(f, "<u8" if f.endswith("_ns") else "<u4") for f in k["fields"]])
    for case in k["cases"]:
        rows = np.array([tuple(r) for r in case["spans"]], dt)
        full = np.zeros(len(rows), ref.REF_DTYPE)
        for f in k["fields"]:
            full[f] = rows[f]
        off = np.array([0, len(rows)], np.uint64)
        s, t, w = host_fold(c.h, off, to_spans(full))
        assert t.tolist() == case["table"], case["name"]
        assert ((s["status"] & native.SPAN_CRITICAL) != 0).astype(int).tolist() == case["critical"]
        assert int(w[0]) == case["trace_wait"]
        bits, rt, rw = cref.fold(c.sg, full, off, n_positions(c.sg))
        assert rt.tolist() == case["table"] and int(rw[0]) == case["trace_wait"]


def test_halves_merged_equal_the_whole():
    c = case_of("zero_hold_mix", isim.MODE_A, 300_000)
    rows = reference("zero_hold_mix", isim.MODE_A, 300_000)
    off, spans = offsets(rows), to_spans(rows)
    _, whole, _ = host_fold(c.h, off, spans)
    half = (len(off) - 1) // 2
    cut = int(off[half])
    _, t1, _ = host_fold(c.h, off[:half + 1], spans[:cut])
    _, t2, _ = host_fold(c.h, off[half:] - off[half], spans[cut:])
    a, b = isim.DesCriticalPath(c.h, t1.copy()), isim.DesCriticalPath(c.h, t2.copy())
    assert a.merge(b) is a and np.array_equal(a.table, whole) and np.array_equal(b.table, t2)
    # a table that starts non-zero is added into
    _, acc, _ = host_fold(c.h, off[half:] - off[half], spans[cut:], table=t1)
    assert np.array_equal(acc, whole)
    rows_ = a.rows()
    assert [r["path_ns"] for r in rows_] == sorted((r["path_ns"] for r in rows_), reverse=True)
    assert abs(sum(r["share"] for r in rows_) - 1.0) < 1e-9
    assert len(a.to_text().splitlines()) == 2 + len(rows_)
    # to_text() stars the critical spans and no other: a trace with a span off the path
    folded = host_fold(c.h, off, spans)[0]
    crit = (folded["status"] & native.SPAN_CRITICAL) != 0
    i = next(i for i in range(len(off) - 1) if not crit[int(off[i]):int(off[i + 1])].all())
    tr = isim.DesTrace(BEGIN + i, folded[int(off[i]):int(off[i + 1])], a.names)
    lines = tr.to_text().splitlines()[1:]
    assert [ln.endswith(" *") for ln in lines] == crit[int(off[i]):int(off[i + 1])].tolist() and lines[0].endswith(" *")
    plain = isim.DesTrace(BEGIN, spans[:int(off[1])], a.names).to_text()
    assert " *" not in plain


def _einval(rc, match):
    assert rc == native.EINVAL and match in native.last_error(), native.last_error()


def test_refusals_need_no_gpu():
    lib = native.load()
    items, static = _handlers()
    buf = np.zeros(64, np.uint64)   # never dereferenced by a refused call
    a = buf.ctypes.data
    assert a % 16 == 0
    w = C.c_uint64()
    native.check(lib.isim_des_critical_path_table_words(items._h, C.byref(w)))
    assert w.value == (items.info.n_services + 1) * native.DCP_ROW_WORDS == 8 * (items.info.n_services + 1)
    native.check(lib.isim_des_critical_path_workspace_bytes(items._h, 1000, C.byref(w)))
    assert w.value == 64 + 16 * 1000

    def dev(h=items, off=a, spans=a, cap=4, info=a, n=4, table=a, wait=a, ws=a, ws_bytes=1 << 20):
        return lib.isim_des_critical_path_device(h._h if h else None, off, spans, cap, info, n, table, wait, ws,
                                                 ws_bytes, None)

    _einval(dev(h=static), "ISIM_FLAG_DYNAMIC")
    _einval(dev(h=None), "null")
    for null in ("off", "info", "table", "spans", "ws"):
        _einval(dev(**{null: None}), "null" if null != "ws" else "workspace")
    for mis in ("off", "info", "table", "wait", "ws"):
        _einval(dev(**{mis: a + 4}), "aligned")
    _einval(dev(spans=a + 8), "aligned")
    _einval(dev(n=(1 << 32) + 1), "2^32")
    _einval(dev(cap=(1 << 40) + 1), "2^40")
    _einval(dev(ws_bytes=64 + 16 * 4 - 1), "workspace")
    for fn in (lib.isim_des_critical_path_table_words,):
        _einval(fn(static._h, C.byref(w)), "ISIM_FLAG_DYNAMIC")
        _einval(fn(items._h, None), "null")
    _einval(lib.isim_des_critical_path_workspace_bytes(static._h, 4, C.byref(w)), "ISIM_FLAG_DYNAMIC")
    _einval(lib.isim_des_critical_path_workspace_bytes(items._h, (1 << 40) + 1, C.byref(w)), "2^40")
    _einval(lib.isim_des_critical_path_workspace_bytes(items._h, 4, None), "null")
    _einval(lib.isim_des_critical_path_merge(items._h, a, None), "null")
    _einval(lib.isim_des_critical_path_merge(static._h, a, a), "ISIM_FLAG_DYNAMIC")
    _einval(lib.isim_des_critical_path_host(static._h, a, 0, a, a, a), "ISIM_FLAG_DYNAMIC")
    _einval(lib.isim_des_critical_path_host(items._h, None, 0, a, a, a), "null")
    _einval(lib.isim_des_critical_path_host(items._h, a, 0, a, None, a), "null")
    _einval(lib.isim_des_critical_path_host(items._h, a, (1 << 32) + 1, a, a, a), "2^32")
    _einval(lib.isim_des_critical_path_host(items._h, a, 0, a + 8, a, a), "aligned")
    _einval(lib.isim_des_critical_path_host(items._h, a, 0, a, a, a + 4), "aligned")
    one = np.array([0, 1], np.uint64)
    _einval(lib.isim_des_critical_path_host(items._h, one.ctypes.data, 1, None, a, None), "null spans")
    _einval(lib.isim_des_critical_path(0, static._h, a, 0, a, a, a), "ISIM_FLAG_DYNAMIC")
    _einval(lib.isim_des_critical_path(0, items._h, None, 0, a, a, a), "null")
    _einval(lib.isim_des_critical_path(0, items._h, a, (1 << 32) + 1, a, a, a), "2^32")


def corruptions(c, off, spans):
    """(name, offsets, spans, refused list entries) over a copy each: trace 3 of the list is damaged."""
    lo = int(off[3])
    m = int(off[4]) - lo
    assert m >= 3
    out = []

    def one(name, field, j, value):
        s = spans.copy()
        s[field][lo + j] = value
        out.append((name, off.copy(), s, [3]))

    one("a wrong hop", "hop", 1, 2)
    one("a forward caller_hop", "caller_hop", 1, 2)
    one("S < a", "start_ns", 1, int(spans["arrival_ns"][lo + 1]) - 1)
    one("F < S", "finish_ns", m - 1, int(spans["start_ns"][lo + m - 1]) - 1)
    one("a child's arrival off by one", "arrival_ns", 1, int(spans["arrival_ns"][lo + 1]) - 1)
    one("a position out of range", "position", m - 1, c.h.info.hops_upper + (1 << 20))
    one("a service out of range", "service", m - 1, c.h.info.n_services)
    o = off.copy()
    o[3], o[4] = off[4], off[3]     # offsets out of order: entries 2 and 4 reach into 3's spans, 3 runs backwards
    out.append(("offsets out of order", o, spans.copy(), [2, 3, 4]))
    return out


@functools.lru_cache(maxsize=None)
def corruption_base():
    c = case_of("zero_hold_mix", isim.MODE_A, 300_000)
    rows = reference("zero_hold_mix", isim.MODE_A, 300_000)
    off = offsets(rows)
    # the first eight traces with at least three spans each
    keep = [i for i in range(len(off) - 1) if off[i + 1] - off[i] >= 3][:8]
    spans = np.concatenate([to_spans(rows[int(off[i]):int(off[i + 1])]) for i in keep])
    noff = np.concatenate([[0], np.cumsum([int(off[i + 1] - off[i]) for i in keep])]).astype(np.uint64)
    return c, noff, spans


def check_corruption(c, off, spans, bad, refused, got):
    """got = (spans, table, waits) of a fold of the damaged list: the refused entries are counted and left
    untouched, the others folded as in the clean list."""
    s, t, w = got
    _, clean_off, clean = corruption_base()
    cs, _, cw = host_fold(c.h, clean_off, clean)
    ns = c.h.info.n_services
    n = len(off) - 1
    assert int(t[ns, native.DCP_H_REFUSED]) == len(refused) and int(t[ns, native.DCP_H_TRACES]) == n - len(refused)
    want_t = np.zeros_like(t)
    for i in range(n):
        lo, hi = int(clean_off[i]), int(clean_off[i + 1])
        if i in refused:
            assert w[i] == U64_MAX
            continue
        assert np.array_equal(s[lo:hi], cs[lo:hi]) and w[i] == cw[i]
        want_t += host_fold(c.h, np.array([0, hi - lo], np.uint64), clean[lo:hi])[1]
    want_t[ns, native.DCP_H_REFUSED] = len(refused)
    assert np.array_equal(t, want_t)
    for i in refused:       # a refused trace's own spans are as they were handed in
        lo, hi = int(clean_off[i]), int(clean_off[i + 1])
        assert np.array_equal(s[lo:hi], bad[lo:hi])


def test_corrupted_spans_are_refused_and_left_untouched():
    c, off, spans = corruption_base()
    for name, o, bad, refused in corruptions(c, off, spans):
        got = host_fold(c.h, o, bad)
        check_corruption(c, o, bad, bad, refused, got)
        # the restatement refuses the same traces
        rows = np.zeros(len(bad), ref.REF_DTYPE)
        for f in ("arrival_ns", "start_ns", "finish_ns", "hop_ns", "hop", "caller_hop", "position", "service", "status"):
            rows[f] = bad[f]
        rows["site"] = bad["slot"]
        _, rt, rw = cref.fold(c.sg, rows, o, n_positions(c.sg))
        assert np.array_equal(rw == U64_MAX, got[2] == U64_MAX), name
