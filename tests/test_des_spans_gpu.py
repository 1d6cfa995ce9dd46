"""DES trace spans on the GPU: the tap on an item-engine batch
(isim_serve_des_spans_device) against the pinned Python restatement
(tests/des_spans_ref.py, pinned by tests/test_des_spans.py), field by field;
the static fields against isim_trace_spans_host; the wait table against the
same call's DES table; the timing invariants; the selection; a NULL tap against
isim_serve_des_device; accumulation, merge and dirty buffers; DesHandler.serve_spans."""
import ctypes as C
import functools

import numpy as np
import pytest

import isim
from isim import native
from isim.des_spans import make_tap

import des_spans_ref as ref
from test_des_spans import case_of, reference

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
W = native.FLAG_TREE_WIDE
MEAN = 300_000
BATCHES = [(1000, 1500), ((1 << 32) - 300, 601)]
# a cyclic schedule, a replicated service, mode B, a forced wide tree, u64 time
GRAPHS = [("canonical_p50", isim.MODE_A, 0), ("tree_reps_p70", isim.MODE_A, 0), ("seq_tree_abort", isim.MODE_B, 0),
          ("mesh_des", isim.MODE_A, W), ("real300seq_t64", isim.MODE_A, 0)]
SMALL = ("zero_hold_mix", isim.MODE_A, 0)       # the selection and accumulation tests
ERRORS = ("zero_hold_mix_b", isim.MODE_B, 0)    # a graph with errors: the classes


def run_tap(c, begin, n, min_latency_ns=0, q_ppm=0, cls=native.Q_ALL, max_traces=None, cap_spans=None, wait=None,
            tap=True, d=None):
    """One device call with dirty (0xFF) tap buffers; wait: the table to add into (zeros when None)."""
    import torch
    d = d or c.d
    max_traces = n if max_traces is None else max_traces
    cap_spans = min(n * int(c.h.info.hops_upper), 1 << 20) if cap_spans is None else cap_spans
    dev = "cuda"
    ws = torch.zeros(d.workspace_bytes(n) + 8, dtype=torch.uint8, device=dev)
    stats = torch.zeros(len(c.h.new_stats()), dtype=torch.int64, device=dev)
    table = torch.zeros(max(1, d.table_words), dtype=torch.int64, device=dev)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    ids = torch.full((max(1, max_traces),), -1, dtype=torch.int64, device=dev)
    off = torch.full((max_traces + 1,), -1, dtype=torch.int64, device=dev)
    spans = torch.full((max(1, cap_spans) * 8,), -1, dtype=torch.int64, device=dev)
    info = torch.full((native.DES_SPAN_INFO_WORDS,), -1, dtype=torch.int64, device=dev)
    words = (c.h.info.n_services + 1) * native.DW_ROW_WORDS
    wt = torch.zeros(words, dtype=torch.int64, device=dev)
    if wait is not None:
        wt.copy_(torch.from_numpy(np.ascontiguousarray(wait, np.uint64).view(np.int64).ravel()))
    t = make_tap(min_latency_ns, q_ppm, cls, max_traces, cap_spans, ids.data_ptr(), off.data_ptr(), spans.data_ptr(),
                 info.data_ptr(), wt.data_ptr()) if tap else None
    s = torch.cuda.current_stream().cuda_stream
    d.serve_spans_device(begin, n, rec.data_ptr(), stats.data_ptr(), table.data_ptr(), ws.data_ptr(), ws.numel(), t, s)
    torch.cuda.synchronize()
    u64 = lambda x: x.cpu().numpy().view(np.uint64)  # noqa: E731
    out = dict(recs=rec.cpu().numpy().view(isim.REC_DTYPE), stats=u64(stats), table=u64(table), ids=u64(ids),
               off=u64(off), spans=spans.cpu().numpy().view(isim.DES_SPAN_DTYPE)[:max(1, cap_spans)], info=u64(info),
               wait=u64(wt).reshape(-1, native.DW_ROW_WORDS))
    return out


@functools.lru_cache(maxsize=None)
def whole(name, mode, flags, begin, n):
    """The whole batch tapped (threshold 0, every trace, room for every span): one call shared by the tests."""
    c = case_of(name, mode, MEAN, flags)
    r = run_tap(c, begin, n)
    total = int(r["off"][n])
    assert list(r["info"]) == [total, n, n, n, n]
    assert np.array_equal(r["ids"], np.arange(begin, begin + n, dtype=np.uint64))
    return c, r, r["spans"][:total]


PARAMS = [(g, b) for g in GRAPHS for b in BATCHES]
IDS = [f"{g[0]}-{b[1]}" for g, b in PARAMS]


@pytest.mark.parametrize("graph,batch", PARAMS, ids=IDS)
def test_spans_equal_the_restatement(gpu, graph, batch):
    c, r, s = whole(*graph, *batch)
    want = reference(graph[0], graph[1], MEAN, *batch)
    assert len(s) == len(want)
    assert np.array_equal(np.diff(r["off"][:batch[1] + 1].astype(np.int64)), r["recs"]["hops"])
    for f in ("arrival_ns", "start_ns", "finish_ns", "hop_ns", "hop", "caller_hop", "position", "service", "status",
              "replica"):
        bad = np.flatnonzero(s[f] != want[f])
        assert bad.size == 0, (f, bad[:4], s[bad[:4]], want[bad[:4]])
    entry = s["hop"] == 0
    assert np.all(s["slot"][entry] == NONE) and not s["reserved"].any()
    assert np.array_equal(c.h.slot_site[s["slot"][~entry]], want["site"][~entry].astype(np.int32))
    assert int((s["start_ns"] > s["arrival_ns"]).sum()) > 0  # contended: some invocation waited


@pytest.mark.parametrize("graph", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_static_fields_equal_the_walk_spans(gpu, graph):
    begin, n = BATCHES[0]
    c, r, s = whole(*graph, begin, n)
    off, host, info = isim.TraceSpans(c.h).raw_host(np.arange(begin, begin + n, dtype=np.uint64))
    assert int(info[native.SPAN_WRITTEN]) == n and np.array_equal(off, r["off"][:n + 1])
    for f in ("hop", "caller_hop", "position", "slot", "service", "status", "hop_ns"):
        assert np.array_equal(s[f], host[f]), f


@pytest.mark.parametrize("graph,batch", PARAMS, ids=IDS)
def test_whole_batch_table_equals_the_des_table(gpu, graph, batch):
    c, r, s = whole(*graph, *batch)
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
    assert list(wt[ns]) == [batch[1], len(s), int(r["recs"]["latency_ns"].sum()), int(w[entry].sum()), 0, 0]


@pytest.mark.parametrize("graph,batch", PARAMS, ids=IDS)
def test_invariants_on_every_span(gpu, graph, batch):
    c, r, s = whole(*graph, *batch)
    begin, n = batch
    a, S, F = s["arrival_ns"], s["start_ns"], s["finish_ns"]
    assert np.all(a <= S) and np.all(S <= F)
    first = r["off"][:n].astype(np.int64)
    trace = np.repeat(np.arange(n), np.diff(r["off"][:n + 1].astype(np.int64)))
    child = s["hop"] != 0
    caller = first[trace[child]] + s["caller_hop"][child].astype(np.int64)
    assert np.all(a[child] >= S[caller] + s["hop_ns"][child]) and np.all(F[child] <= F[caller])
    assert np.array_equal(F[first] - a[first], r["recs"]["latency_ns"])
    assert np.array_equal(a[first], c.d.arrivals(begin, n))
    # one worker per (service, replica): the holds [S, S + P_s) do not overlap and start in (a, trace, hop) order
    hold = np.array(ref.holds(c.sg), np.uint64)[s["service"]]
    order = np.lexsort((s["hop"], trace, a, s["replica"], s["service"]))
    same = (s["service"][order][1:] == s["service"][order][:-1]) & (s["replica"][order][1:] == s["replica"][order][:-1])
    So, ho = S[order], hold[order]
    assert np.all(So[1:][same] >= (So[:-1] + ho[:-1])[same])


@functools.lru_cache(maxsize=None)
def small_whole(graph=SMALL):
    return whole(*graph, *BATCHES[0])


def _check_selected(c, r, whole_r, whole_spans, want, max_traces):
    """r chose `want` (positions in the batch, ascending), cut at max_traces: info, ids, offsets and spans."""
    begin = BATCHES[0][0]
    kept = want[:max_traces]
    woff = whole_r["off"].astype(np.int64)
    cnt = woff[kept + 1] - woff[kept]
    total = int(cnt.sum())
    assert list(r["info"]) == [total, len(kept), len(kept), len(kept), len(want)]
    assert np.array_equal(r["ids"][:len(kept)], kept.astype(np.uint64) + np.uint64(begin))
    assert np.array_equal(r["off"][:len(kept) + 1], np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64))
    got = r["spans"][:total]
    exp = np.concatenate([whole_spans[woff[t]:woff[t + 1]] for t in kept]) if len(kept) else whole_spans[:0]
    assert np.array_equal(got, exp)
    # past the list and the written spans the dirty buffers are untouched
    assert np.all(r["ids"][len(kept):] == np.uint64(0xFFFFFFFFFFFFFFFF))
    assert np.all(r["off"][len(kept) + 1:] == np.uint64(0xFFFFFFFFFFFFFFFF))
    assert np.all(r["spans"][total:].view(np.uint8) == 0xFF)
    ns = c.h.info.n_services
    assert int(r["wait"][ns, native.DW_H_TRACES]) == len(kept) and int(r["wait"][ns, native.DW_H_SPANS]) == total
    assert np.array_equal(r["wait"][:ns, native.DW_INVOCATIONS], np.bincount(exp["service"], minlength=ns))
    # the batch itself is the same whatever is tapped
    assert np.array_equal(r["recs"], whole_r["recs"]) and np.array_equal(r["table"], whole_r["table"])


@pytest.mark.parametrize("k", [0, 1, 63, 64, 65, 1000])
def test_threshold_selects(gpu, k):
    c, wr, ws = small_whole()
    begin, n = BATCHES[0]
    lat = wr["recs"]["latency_ns"]
    desc = np.sort(lat)[::-1]
    thr = int(desc[0]) + 1 if k == 0 else int(desc[k - 1])
    want = np.flatnonzero(lat >= np.uint64(thr))
    assert len(want) >= k and (k != 0 or len(want) == 0)
    r = run_tap(c, begin, n, min_latency_ns=thr, max_traces=64, cap_spans=1 << 14)
    _check_selected(c, r, wr, ws, want, 64)


def test_q_ppm_is_the_batch_order_statistic(gpu):
    c, wr, ws = small_whole()
    begin, n = BATCHES[0]
    lat = wr["recs"]["latency_ns"]
    k = C.c_uint64()
    native.check(native.load().isim_quantile_rank(n, 999000, C.byref(k)))
    assert k.value == max(1, -(-999000 * n // 1_000_000))
    thr = np.sort(lat)[k.value - 1]
    want = np.flatnonzero(lat >= thr)
    assert 1 <= len(want) <= 64
    r = run_tap(c, begin, n, min_latency_ns=12345, q_ppm=999000, max_traces=64, cap_spans=1 << 14)
    _check_selected(c, r, wr, ws, want, 64)


@pytest.mark.parametrize("cls", [native.Q_200, native.Q_500])
def test_classes(gpu, cls):
    c, wr, ws = small_whole(ERRORS)
    begin, n = BATCHES[0]
    recs = wr["recs"]
    in_cls = (recs["status_err"] >> 31) == (1 if cls == native.Q_500 else 0)
    assert 10 < int(in_cls.sum()) < n - 10
    # every record of the class, then the upper half of the class by its own median
    r = run_tap(c, begin, n, cls=cls, max_traces=n, cap_spans=1 << 15)
    _check_selected(c, r, wr, ws, np.flatnonzero(in_cls), n)
    lat = np.sort(recs["latency_ns"][in_cls])
    k = C.c_uint64()
    native.check(native.load().isim_quantile_rank(len(lat), 500000, C.byref(k)))
    want = np.flatnonzero(in_cls & (recs["latency_ns"] >= lat[k.value - 1]))
    r = run_tap(c, begin, n, q_ppm=500000, cls=cls, max_traces=n, cap_spans=1 << 15)
    _check_selected(c, r, wr, ws, want, n)


def test_cap_spans_one_short(gpu):
    c, wr, ws = small_whole()
    begin, n = BATCHES[0]
    woff = wr["off"].astype(np.int64)
    total = int(woff[10])
    r = run_tap(c, begin, n, max_traces=10, cap_spans=total - 1)
    assert list(r["info"]) == [total, 9, 10, 9, n]
    assert np.array_equal(r["off"][:11], wr["off"][:11])
    assert np.array_equal(r["spans"][:woff[9]], ws[:woff[9]])
    assert np.all(r["spans"][woff[9]:].view(np.uint8) == 0xFF)   # the unwritten tail is untouched
    ns = c.h.info.n_services
    assert list(r["wait"][ns][:2]) == [9, int(woff[9])]
    assert np.array_equal(r["wait"][:ns, native.DW_INVOCATIONS], np.bincount(ws[:woff[9]]["service"], minlength=ns))
    # no room at all: nothing written, the offsets still say what is needed
    r = run_tap(c, begin, n, max_traces=10, cap_spans=0)
    assert list(r["info"]) == [total, 0, 10, 0, n] and not r["wait"].any()


@pytest.mark.parametrize("profile", [False, True])
def test_null_tap_is_the_existing_call(gpu, profile):
    import torch
    c, _, _ = small_whole()
    begin, n = BATCHES[0]
    d = c.d
    if profile:
        d = isim.DesHandler(c.h, profile=isim.LoadProfile.steps([(40_000_000, 500_000), (20_000_000, 100_000)], 300_000))
    got = run_tap(c, begin, n, tap=False, d=d)
    ws = torch.zeros(d.workspace_bytes(n) + 8, dtype=torch.uint8, device="cuda")
    stats = torch.zeros(len(c.h.new_stats()), dtype=torch.int64, device="cuda")
    table = torch.zeros(max(1, d.table_words), dtype=torch.int64, device="cuda")
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    d.serve_device(begin, n, rec.data_ptr(), stats.data_ptr(), table.data_ptr(), ws.data_ptr(), ws.numel(),
                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(got["recs"], rec.cpu().numpy().view(isim.REC_DTYPE))
    assert np.array_equal(got["stats"], stats.cpu().numpy().view(np.uint64))
    assert np.array_equal(got["table"], table.cpu().numpy().view(np.uint64))
    # and a tap changes none of the three
    tapped = run_tap(c, begin, n, q_ppm=990000, max_traces=64, cap_spans=1 << 14, d=d)
    for f in ("recs", "stats", "table"):
        assert np.array_equal(tapped[f], got[f]), f
    assert int(tapped["info"][native.SPAN_WRITTEN]) > 0


def test_tables_accumulate_and_merge(gpu):
    c, _, _ = small_whole()
    begin, n = BATCHES[0]
    ns = c.h.info.n_services
    h1 = run_tap(c, begin, 750, cap_spans=1 << 15)
    h2 = run_tap(c, begin + 750, 750, cap_spans=1 << 15)
    assert h1["wait"][:ns, native.DW_SUM_WAIT].sum() > 0 and h2["wait"][:ns, native.DW_SUM_WAIT].sum() > 0
    rng = np.random.default_rng(3)
    start = rng.integers(1, 1 << 30, (ns + 1, native.DW_ROW_WORDS), dtype=np.uint64)
    start[:ns, native.DW_MAX_WAIT] = h1["wait"][:ns, native.DW_MAX_WAIT] // 2 + 1   # some maxima win, some lose
    acc = run_tap(c, begin, 750, cap_spans=1 << 15, wait=start)
    acc = run_tap(c, begin + 750, 750, cap_spans=1 << 15, wait=acc["wait"])
    want = isim.DesWaitTable(c.h, start.copy()).merge(isim.DesWaitTable(c.h, h1["wait"].copy())) \
        .merge(isim.DesWaitTable(c.h, h2["wait"].copy()))
    assert np.array_equal(acc["wait"], want.table)


def test_serve_spans_with_a_step_profile(gpu):
    c, _, _ = small_whole()
    prof = isim.LoadProfile.steps([(40_000_000, 500_000), (20_000_000, 100_000)], 300_000)
    d = isim.DesHandler(c.h, profile=prof)
    begin, n = BATCHES[0]
    recs, stats, table, traces, waits = d.serve_spans(begin, n)
    ref_recs, ref_stats, ref_table = d.serve(begin, n)
    assert np.array_equal(recs, ref_recs) and np.array_equal(stats, ref_stats) and np.array_equal(table, ref_table)
    lat = recs["latency_ns"]
    k = max(1, -(-999000 * n // 1_000_000))
    want = np.flatnonzero(lat >= np.sort(lat)[k - 1])
    assert [t.trace_id for t in traces] == [begin + int(i) for i in want[:64]]
    arr = d.arrivals(begin, n)
    for t in traces:
        i = t.trace_id - begin
        assert t.latency_ns == int(lat[i]) and t.arrival_ns == int(arr[i]) and len(t) == int(recs["hops"][i])
        text = t.to_text().splitlines()
        assert len(text) == 1 + len(t) and all("wait=" in line for line in text[1:])
    assert waits.header["traces"] == len(traces) and waits.header["spans"] == sum(len(t) for t in traces)
    assert waits.header["sum_latency_ns"] == sum(t.latency_ns for t in traces)
    assert len(waits.to_text().splitlines()) == 2 + len(waits.rows())
    # min_latency_ns in place of the percentile, added into the same table
    thr = int(np.sort(lat)[-3])
    more = d.serve_spans(begin, n, min_latency_ns=thr, wait_table=waits)
    extra = int((lat >= np.uint64(thr)).sum())
    assert len(more[3]) == extra >= 3 and more[4] is waits and waits.header["traces"] == len(traces) + extra
