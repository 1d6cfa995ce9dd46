"""The service timeline on the GPU: isim_service_timeline_device against
isim_service_timeline_host, word for word, on the tapped whole batches of the DES span tests; the
identities against the wait and DES tables of the same call; the entry service against isim.timeline; span
counts around a wave, one cell for every lane, the 40-deep chain, a 1 ns window with 65536 rows; a dirty
workspace, a non-zero table, two calls, two streams, a captured graph, corrupted spans and
DesHandler.service_timeline."""
import numpy as np
import pytest

import isim
from isim import native
from isim.des_spans import make_tap
from isim.service_timeline import service_timeline_device, service_timeline_table_words, service_timeline_workspace_bytes

import critical_path_graphs as cpg
from test_des_gpu import DesCase
from test_des_spans_gpu import BATCHES, GRAPHS, MEAN, run_tap, small_whole, whole

pytestmark = pytest.mark.gpu

W = native.SVT_ROW_WORDS
# (window_ns, n_windows): 1 ns, 1 us, a window that is no power of two, 2^40
WINDOWS = [(1, 4096), (1000, 4096), (333_333, 300), (1 << 40, 3)]


def t0_of(spans, mid):
    return int(np.sort(spans["arrival_ns"])[len(spans) // 2]) if mid and len(spans) else 0


def device_fold(h, spans, window, n, t0, table=None, calls=1, cap_spans=None, written_spans=None):
    """Uploads the spans as one list entry, folds them `calls` times on the current stream over a 0xFF
    workspace and returns the flat table."""
    import torch
    dev = "cuda"
    cap = len(spans) if cap_spans is None else cap_spans
    end = len(spans) if written_spans is None else written_spans
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).ravel().copy()).to(dev)  # noqa: E731
    d_spans = up(spans) if len(spans) else torch.zeros(8, dtype=torch.int64, device=dev)
    d_off = up(np.array([0, end], np.uint64))
    d_info = up(np.array([end, 1, 1, 1, 1], np.uint64))
    words = service_timeline_table_words(h, window, n, t0)
    d_table = up(table) if table is not None else torch.zeros(words, dtype=torch.int64, device=dev)
    ws_bytes = service_timeline_workspace_bytes(h, window, n, t0)
    ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(calls):
        service_timeline_device(h, window, n, t0, d_off.data_ptr(), d_spans.data_ptr(), cap, d_info.data_ptr(),
                                d_table.data_ptr(), ws.data_ptr(), ws_bytes, s)
    torch.cuda.synchronize()
    return d_table.cpu().numpy().view(np.uint64)[:words]


def same_as_host(h, spans, window, n, t0, table=None):
    got = device_fold(h, spans, window, n, t0, table=table)
    want = isim.service_timeline_host(h, spans, window, n, t0, table=None if table is None else table.copy())
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:4], got[bad[:4]], want[bad[:4]])
    return got


@pytest.mark.parametrize("window", WINDOWS, ids=[f"w{w[0]}" for w in WINDOWS])
@pytest.mark.parametrize("graph", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_device_equals_host(gpu, graph, window):
    begin, n = BATCHES[0]
    c, r, spans = whole(*graph, begin, n)
    for mid in (False, True):
        t = same_as_host(c.h, spans, window[0], window[1], t0_of(spans, mid))
        assert list(t[-W:]) == [len(spans), 0] + [0] * (W - 2)


@pytest.mark.parametrize("graph", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_identities_against_the_wait_and_des_tables(gpu, graph):
    begin, n = BATCHES[0]
    c, r, spans = whole(*graph, begin, n)
    ns = c.h.info.n_services
    hold, reps = isim.service_holds(c.h)
    wt, des = r["wait"], c.d.fold(r["table"])
    for window, nw in WINDOWS:
        for mid in (False, True):
            t = device_fold(c.h, spans, window, nw, t0_of(spans, mid))[:-W].reshape(ns, nw + 2, W)
            assert np.array_equal(t[:, :, native.SVT_ARRIVED].sum(axis=1), wt[:ns, native.DW_INVOCATIONS])
            assert np.array_equal(t[:, :, native.SVT_QUEUED_NS].sum(axis=1), wt[:ns, native.DW_SUM_WAIT])
            assert np.array_equal(t[:, :, native.SVT_SUM_WAIT].sum(axis=1), wt[:ns, native.DW_SUM_WAIT])
            assert np.array_equal(t[:, :, native.SVT_MAX_WAIT].max(axis=1), wt[:ns, native.DW_MAX_WAIT])
            assert np.array_equal(t[:, :, native.SVT_BUSY_NS].sum(axis=1), des[:, native.DES_SUM_HOLD])
            assert np.array_equal(t[:, :, native.SVT_BUSY_NS].sum(axis=1), wt[:ns, native.DW_INVOCATIONS] * hold)
            # one worker per replica: the utilisation of a window never passes 1
            assert np.all(t[:, 1:-1, native.SVT_BUSY_NS] <= np.uint64(window) * reps[:, None].astype(np.uint64))


@pytest.mark.parametrize("graph", GRAPHS[:2], ids=[g[0] for g in GRAPHS[:2]])
def test_the_entry_service_against_the_client_timeline(gpu, graph):
    begin, n = BATCHES[0]
    c, r, spans = whole(*graph, begin, n)
    entry = int(spans["service"][0])
    arr = c.d.arrivals(begin, n)
    for window, nw in WINDOWS[1:3]:
        t0 = t0_of(spans, True)
        tl = isim.timeline_table(arr, r["recs"], window, nw, t0).reshape(nw + 2, native.TL_ROW_WORDS)
        t = device_fold(c.h, spans, window, nw, t0)[:-W].reshape(-1, nw + 2, W)[entry]
        if not np.any((spans["service"] == entry) & (spans["hop"] != 0)):   # the entry service is invoked by the client only
            assert np.array_equal(t[:, native.SVT_ARRIVED], tl[:, native.TL_ARRIVED])
            assert np.array_equal(t[:, native.SVT_FINISHED:native.SVT_FINISHED + 2], tl[:, native.TL_DONE:native.TL_DONE + 2])
        else:
            pytest.fail("the entry service is also a callee: the graph does not fit this test")


@pytest.mark.parametrize("k", [0, 1, 63, 64, 65, 1000])
def test_span_counts(gpu, k):
    c, r, spans = small_whole()
    for window, nw in WINDOWS[:3]:
        t = same_as_host(c.h, spans[:k], window, nw, t0_of(spans[:k], True))
        assert int(t[-W + native.SVT_H_FOLDED]) == k
    # cap_spans only bounds the grid and the count: a longer buffer of which k spans were written, and a
    # list that claims more than the buffer holds
    if k in (1, 65):
        got = device_fold(c.h, spans[:k + 70], 1000, 4096, 0, written_spans=k)
        assert np.array_equal(got, isim.service_timeline_host(c.h, spans[:k], 1000, 4096, 0))
        got = device_fold(c.h, spans[:k], 1000, 4096, 0, written_spans=k + 70)
        assert np.array_equal(got, isim.service_timeline_host(c.h, spans[:k], 1000, 4096, 0))


def test_one_service_every_lane_on_one_cell(gpu):
    c = DesCase({"services": [{"name": "a", "isEntrypoint": True, "script": [{"sleep": "200us"}]}]}, 150_000,
                flags=native.FLAG_DYNAMIC)
    r = run_tap(c, 0, 200)
    spans = r["spans"][:200]
    assert int(r["off"][200]) == 200 and int((spans["start_ns"] > spans["arrival_ns"]).sum()) > 0
    for window, nw in [(1 << 40, 1), (10_000_000, 4), (1000, 4096), (1, 65536)]:
        t = same_as_host(c.h, spans, window, nw, 0)
        assert int(t[:-W].reshape(nw + 2, W)[:, native.SVT_BUSY_NS].sum()) == 200 * 200_000


def test_the_40_deep_chain(gpu):
    c = DesCase(cpg.chain(40), MEAN, flags=native.FLAG_DYNAMIC)
    n = 300
    r = run_tap(c, 0, n)
    spans = r["spans"][:int(r["off"][n])]
    assert len(spans) > n      # long, thin traces: probabilistic calls cut most of them short of 40
    for window, nw in WINDOWS[1:3]:
        same_as_host(c.h, spans, window, nw, t0_of(spans, True))


def test_a_1ns_window_with_65536_rows(gpu):
    """Long interiors: a wait of microseconds covers thousands of 1 ns rows and runs into "after"."""
    c, r, spans = small_whole()
    t0 = t0_of(spans, True)
    t = same_as_host(c.h, spans, 1, 65536, t0)
    ns = c.h.info.n_services
    rows = t[:-W].reshape(ns, 65538, W)
    assert int(rows[:, 1:-1, native.SVT_BUSY_NS].max()) >= 1 and int(rows[:, -1, native.SVT_BUSY_NS].sum()) > 0


def test_a_table_that_starts_non_zero_and_two_calls(gpu):
    c, r, spans = small_whole()
    window, nw, t0 = 333_333, 300, t0_of(spans, True)
    words = service_timeline_table_words(c.h, window, nw, t0)
    rng = np.random.default_rng(11)
    start = rng.integers(1, 1 << 62, words, dtype=np.uint64)
    one = isim.service_timeline_host(c.h, spans, window, nw, t0)
    mx = np.zeros(words, bool)
    mx[:-W][native.SVT_MAX_WAIT::W] = True
    start[mx] = one[mx] // 2 + 1     # some maxima win, some lose
    same_as_host(c.h, spans, window, nw, t0, table=start)
    # two calls double every word except MAX_WAIT
    twice = device_fold(c.h, spans, window, nw, t0, calls=2)
    assert np.array_equal(twice, np.where(mx, one, one * np.uint64(2)))


def tap_buffers(c, n, window, nw, t0, cap_spans=None):
    import torch
    dev = "cuda"
    cap = n * int(c.h.info.hops_upper) if cap_spans is None else cap_spans
    z = lambda k, fill=0: torch.full((max(1, k),), fill, dtype=torch.int64, device=dev)  # noqa: E731
    b = dict(ws=z(c.d.workspace_bytes(n) // 8 + 1), stats=z(len(c.h.new_stats())), table=z(c.d.table_words),
             rec=z(2 * n), ids=z(n, -1), off=z(n + 1, -1), spans=z(8 * cap, -1), info=z(native.DES_SPAN_INFO_WORDS, -1),
             out=z(service_timeline_table_words(c.h, window, nw, t0)),
             tws=z(service_timeline_workspace_bytes(c.h, window, nw, t0) // 8, -1), cap=cap)
    b["tap"] = make_tap(0, 0, native.Q_ALL, n, cap, b["ids"].data_ptr(), b["off"].data_ptr(), b["spans"].data_ptr(),
                        b["info"].data_ptr(), 0)
    return b


def fold_call(c, b, window, nw, t0, stream):
    service_timeline_device(c.h, window, nw, t0, b["off"].data_ptr(), b["spans"].data_ptr(), b["cap"],
                            b["info"].data_ptr(), b["out"].data_ptr(), b["tws"].data_ptr(), b["tws"].numel() * 8, stream)


def check_tapped(c, b, n, window, nw, t0, folds=1):
    u64 = lambda x: x.cpu().numpy().view(np.uint64)  # noqa: E731
    info, off = u64(b["info"]), u64(b["off"])
    assert int(info[native.SPAN_WRITTEN]) == n
    spans = b["spans"].cpu().numpy().view(isim.DES_SPAN_DTYPE)[:int(off[n])]
    want = isim.service_timeline_host(c.h, spans, window, nw, t0)
    mx = np.zeros(want.size, bool)
    mx[:-W][native.SVT_MAX_WAIT::W] = True
    assert np.array_equal(u64(b["out"])[:want.size], np.where(mx, want, want * np.uint64(folds)))


def test_tap_and_fold_on_two_streams(gpu):
    import torch
    c, _, _ = small_whole()
    begin, n = BATCHES[0]
    window, nw, t0 = 1000, 4096, 100_000_000
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    bufs = [tap_buffers(c, n, window, nw, t0) for _ in streams]
    torch.cuda.synchronize()
    for k, (st, b) in enumerate(zip(streams, bufs)):
        with torch.cuda.stream(st):
            c.d.serve_spans_device(begin + k * n, n, b["rec"].data_ptr(), b["stats"].data_ptr(), b["table"].data_ptr(),
                                   b["ws"].data_ptr(), b["ws"].numel() * 8, b["tap"], st.cuda_stream)
            fold_call(c, b, window, nw, t0, st.cuda_stream)
    torch.cuda.synchronize()
    for b in bufs:
        check_tapped(c, b, n, window, nw, t0)


def test_the_fold_captured_in_a_graph(gpu):
    import torch
    c, _, _ = small_whole()
    begin, n = BATCHES[0]
    window, nw, t0 = 1000, 4096, 100_000_000
    b = tap_buffers(c, n, window, nw, t0)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c.d.serve_spans_device(begin, n, b["rec"].data_ptr(), b["stats"].data_ptr(), b["table"].data_ptr(),
                               b["ws"].data_ptr(), b["ws"].numel() * 8, b["tap"], st.cuda_stream)
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            fold_call(c, b, window, nw, t0, st.cuda_stream)
        for _ in range(3):
            g.replay()
    torch.cuda.synchronize()
    check_tapped(c, b, n, window, nw, t0, folds=3)


def test_corrupted_spans_are_refused_as_on_the_host(gpu):
    c, r, spans = small_whole()
    ns = c.h.info.n_services
    m = min(2000, len(spans))
    assert m >= 1000
    bad = spans[:m].copy()
    rng = np.random.default_rng(5)
    pick = rng.permutation(m)
    bad["service"][pick[:100]] = ns
    bad["service"][pick[100:200]] = 0xFFFFFFFF
    bad["start_ns"][pick[200:300]] = bad["arrival_ns"][pick[200:300]] - 1
    bad["finish_ns"][pick[300:400]] = bad["start_ns"][pick[300:400]] - 1
    bad["start_ns"][pick[400:450]] = 0xFFFFFFFFFFFFFFFF
    for window, nw in WINDOWS[1:3]:
        t = same_as_host(c.h, bad, window, nw, t0_of(spans, True))
        assert int(t[-W + native.SVT_H_REFUSED]) >= 400 and int(t[-W + native.SVT_H_FOLDED]) + int(t[-W + native.SVT_H_REFUSED]) == m
        keep = np.ones(m, bool)
        keep[pick[:450]] = False
        clean = isim.service_timeline_host(c.h, bad[keep], window, nw, t0_of(spans, True))
        assert np.array_equal(t[:-W], clean[:-W])      # a refused span adds to nothing else


def test_handler_service_timeline_with_a_step_profile(gpu):
    c, _, _ = small_whole()
    prof = isim.LoadProfile.steps([(40_000_000, 500_000), (20_000_000, 100_000)], 300_000)
    d = isim.DesHandler(c.h, profile=prof)
    begin, n = BATCHES[0]
    window, nw = 1_000_000, 200
    t = d.service_timeline(begin, n, window, nw)
    assert isinstance(t, isim.ServiceTimeline)
    recs, stats, table, traces, waits = d.serve_spans(begin, n, min_latency_ns=0, max_traces=n,
                                                      cap_spans=n * int(c.h.info.hops_upper))
    assert len(traces) == n
    spans = np.concatenate([x.spans for x in traces])
    assert np.array_equal(t.flat, isim.service_timeline_host(c.h, spans, window, nw, 0))
    assert t.header == {"folded": len(spans), "refused": 0}
    assert len(t.to_text(top=3).splitlines()) == 5 and 0.0 < t.utilisation().max() <= 1.0
    # added into the same table: a second batch
    again = d.service_timeline(begin + n, n, window, nw, into=t)
    assert again is t and t.header["folded"] > len(spans)
    # a cap that is too small raises: never a partial table
    before = t.flat.copy()
    with pytest.raises(RuntimeError):
        d.service_timeline(begin, n, window, nw, into=t, cap_spans=len(spans) - 1)
    assert np.array_equal(t.flat, before)
