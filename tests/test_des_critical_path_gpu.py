"""DES critical path on the GPU: isim_des_critical_path_device
against isim_des_critical_path_host on the spans the tap wrote: spans byte for
byte, table word for word, d_trace_wait value for value; list lengths, a trace
of one span and traces of more than 64, a short cap, a dirty workspace, a
non-zero table, two streams, a captured graph, corrupted spans and
DesHandler.serve_spans(critical_path=True)."""
import functools

import numpy as np
import pytest

import isim
from isim import native
from isim.des_spans import critical_path_workspace_bytes, des_critical_path_device, make_tap

import critical_path_graphs as cpg
from test_des_critical_path import U64_MAX, check_corruption, corruption_base, corruptions, host_fold
from test_des_gpu import DesCase
from test_des_spans_gpu import BATCHES, GRAPHS, MEAN, run_tap, small_whole, whole

pytestmark = pytest.mark.gpu

SENTINEL = np.uint64(0x1111)


def invariant(c, t):
    ns = c.h.info.n_services
    part = t[:ns, native.DCP_WAIT_NS] + t[:ns, native.DCP_SELF_NS] + t[:ns, native.DCP_HOP_NS]
    assert int(part.sum(dtype=np.uint64)) == int(t[ns, native.DCP_H_SUM_LATENCY])
    assert not t[ns, 5:].any()


def device_fold(c, off, spans, written, n_ids=None, cap_spans=None, table=None, calls=1):
    """Uploads a list, folds it `calls` times on the current stream over a 0xFF workspace; returns the spans,
    the table and d_trace_wait (dirty with SENTINEL before the call)."""
    import torch
    n_ids = len(off) - 1 if n_ids is None else n_ids
    cap_spans = len(spans) if cap_spans is None else cap_spans
    dev = "cuda"
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).ravel().copy()).to(dev)  # noqa: E731
    d_off = up(np.ascontiguousarray(off, np.uint64))
    d_spans = up(spans) if len(spans) else torch.zeros(8, dtype=torch.int64, device=dev)
    d_info = up(np.array([int(off[written]), written, n_ids, written, written], np.uint64))
    words = (c.h.info.n_services + 1) * native.DCP_ROW_WORDS
    d_table = up(table) if table is not None else torch.zeros(words, dtype=torch.int64, device=dev)
    d_wait = up(np.full(max(1, n_ids), SENTINEL, np.uint64))
    ws_bytes = critical_path_workspace_bytes(c.h, cap_spans)
    ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(calls):
        des_critical_path_device(c.h, d_off.data_ptr(), d_spans.data_ptr(), cap_spans, d_info.data_ptr(), n_ids,
                                 d_table.data_ptr(), d_wait.data_ptr(), ws.data_ptr(), ws_bytes, s)
    torch.cuda.synchronize()
    u64 = lambda x: x.cpu().numpy().view(np.uint64)  # noqa: E731
    return (d_spans.cpu().numpy().view(isim.DES_SPAN_DTYPE)[:len(spans)], u64(d_table).reshape(-1, native.DCP_ROW_WORDS),
            u64(d_wait)[:n_ids])


def same_as_host(c, off, spans, written=None, table=None):
    written = len(off) - 1 if written is None else written
    s, t, w = device_fold(c, off, spans, written, table=table)
    hs, ht, hw = host_fold(c.h, off, spans, table=table, n=written)
    assert np.array_equal(s.view(np.uint8), hs.view(np.uint8))
    assert np.array_equal(t, ht), (t, ht)
    assert np.array_equal(w[:written], hw) and np.all(w[written:] == SENTINEL)
    if table is None:
        invariant(c, t)
    return s, t, w


@pytest.mark.parametrize("graph", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_device_equals_host(gpu, graph):
    begin, n = BATCHES[0]
    c, r, spans = whole(*graph, begin, n)
    s, t, w = same_as_host(c, r["off"][:n + 1], spans)
    ns = c.h.info.n_services
    assert int(t[ns, native.DCP_H_TRACES]) == n and int(t[ns, native.DCP_H_REFUSED]) == 0
    assert int(t[:ns, native.DCP_WAIT_NS].sum()) > 0         # contended: queueing is on some critical path
    assert np.array_equal(t[ns, native.DCP_H_SUM_LATENCY], r["recs"]["latency_ns"].sum(dtype=np.uint64))


@functools.lru_cache(maxsize=None)
def chain_whole():
    """The 40-deep chain under the DES: long, thin traces, many of more than 64 spans."""
    c = DesCase(cpg.chain(40), MEAN, flags=native.FLAG_DYNAMIC)
    assert c.d.info.items == 1
    n = 1000
    r = run_tap(c, 0, n)
    return c, r, r["spans"][:int(r["off"][n])], n


def test_the_40_deep_chain_strides(gpu):
    c, r, spans, n = chain_whole()
    assert int(np.diff(r["off"][:n + 1].astype(np.int64)).max()) > 64
    same_as_host(c, r["off"][:n + 1], spans)


def test_a_trace_of_one_span(gpu):
    c = DesCase({"services": [{"name": "a", "isEntrypoint": True, "script": [{"sleep": "200us"}]}]}, 150_000,
                flags=native.FLAG_DYNAMIC)
    assert c.d.info.items == 1
    r = run_tap(c, 0, 200)
    assert int(r["off"][200]) == 200
    s, t, w = same_as_host(c, r["off"][:201], r["spans"][:200])
    assert np.all(s["status"] & native.SPAN_CRITICAL) and int(t[0, native.DCP_WAIT_NS]) == int(w.sum()) > 0


@pytest.mark.parametrize("k", [0, 1, 63, 64, 65, 1000])
def test_list_lengths(gpu, k):
    c, r, spans = small_whole()
    off = r["off"][:k + 1]
    same_as_host(c, off, spans[:int(off[k])])
    # n_ids only bounds the grid: a longer list of which k entries were written
    if k in (1, 65):
        s, t, w = device_fold(c, r["off"][:k + 9], spans[:int(off[k])], k, n_ids=k + 8)
        hs, ht, hw = host_fold(c.h, off, spans[:int(off[k])])
        assert np.array_equal(s, hs) and np.array_equal(t, ht) and np.array_equal(w[:k], hw) and np.all(w[k:] == SENTINEL)
        invariant(c, t)


def test_cap_one_span_short(gpu):
    c, wr, ws = small_whole()
    begin, n = BATCHES[0]
    total = int(wr["off"][10])
    r = run_tap(c, begin, n, max_traces=10, cap_spans=total - 1)     # nine traces fit
    assert list(r["info"][:4]) == [total, 9, 10, 9]
    s, t, w = device_fold(c, r["off"][:11], r["spans"], 9, n_ids=10, cap_spans=total - 1)
    hs, ht, hw = host_fold(c.h, r["off"][:10], r["spans"][:int(r["off"][9])])
    assert np.array_equal(s[:int(r["off"][9])], hs) and np.array_equal(t, ht) and np.array_equal(w[:9], hw)
    assert w[9] == SENTINEL and np.all(s[int(r["off"][9]):].view(np.uint8) == 0xFF)   # the unwritten tail is untouched
    invariant(c, t)


def test_a_table_that_starts_non_zero(gpu):
    c, r, spans = small_whole()
    rng = np.random.default_rng(7)
    start = rng.integers(1, 1 << 62, ((c.h.info.n_services + 1), native.DCP_ROW_WORDS), dtype=np.uint64)
    same_as_host(c, r["off"][:301], spans[:int(r["off"][300])], table=start)


def tap_buffers(c, n, max_traces, cap_spans):
    import torch
    dev = "cuda"
    z = lambda k, fill=0: torch.full((max(1, k),), fill, dtype=torch.int64, device=dev)  # noqa: E731
    b = dict(ws=z(c.d.workspace_bytes(n) // 8 + 1), stats=z(len(c.h.new_stats())), table=z(c.d.table_words),
             rec=z(2 * n), ids=z(max_traces, -1), off=z(max_traces + 1, -1), spans=z(8 * cap_spans, -1),
             info=z(native.DES_SPAN_INFO_WORDS, -1), cpt=z((c.h.info.n_services + 1) * native.DCP_ROW_WORDS),
             tw=z(max_traces, int(SENTINEL)), cws=z(critical_path_workspace_bytes(c.h, cap_spans) // 8, -1))
    b["tap"] = make_tap(0, 990000, native.Q_ALL, max_traces, cap_spans, b["ids"].data_ptr(), b["off"].data_ptr(),
                        b["spans"].data_ptr(), b["info"].data_ptr(), 0)
    return b


def fold_call(c, b, max_traces, cap_spans, stream):
    des_critical_path_device(c.h, b["off"].data_ptr(), b["spans"].data_ptr(), cap_spans, b["info"].data_ptr(),
                             max_traces, b["cpt"].data_ptr(), b["tw"].data_ptr(), b["cws"].data_ptr(),
                             b["cws"].numel() * 8, stream)


def check_tapped(c, b, folds=1):
    u64 = lambda x: x.cpu().numpy().view(np.uint64)  # noqa: E731
    info, off = u64(b["info"]), u64(b["off"])
    written = int(info[native.SPAN_WRITTEN])
    assert written > 0
    spans = b["spans"].cpu().numpy().view(isim.DES_SPAN_DTYPE)[:int(off[written])]
    clean = spans.copy()
    clean["status"] &= ~np.uint32(native.SPAN_CRITICAL)
    hs, ht, hw = host_fold(c.h, off[:written + 1], clean)
    assert np.array_equal(spans, hs) and np.array_equal(u64(b["tw"])[:written], hw)
    assert np.array_equal(u64(b["cpt"]).reshape(ht.shape), ht * np.uint64(folds))
    invariant(c, ht)
    return written


def test_tap_and_fold_on_two_streams(gpu):
    import torch
    c, _, _ = small_whole()
    begin, n = BATCHES[0]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    bufs = [tap_buffers(c, n, 64, 1 << 14) for _ in streams]
    torch.cuda.synchronize()
    for k, (st, b) in enumerate(zip(streams, bufs)):
        with torch.cuda.stream(st):
            c.d.serve_spans_device(begin + k * n, n, b["rec"].data_ptr(), b["stats"].data_ptr(), b["table"].data_ptr(),
                                   b["ws"].data_ptr(), b["ws"].numel() * 8, b["tap"], st.cuda_stream)
            fold_call(c, b, 64, 1 << 14, st.cuda_stream)
    torch.cuda.synchronize()
    for b in bufs:
        check_tapped(c, b)


def test_the_fold_captured_in_a_graph(gpu):
    import torch
    c, _, _ = small_whole()
    begin, n = BATCHES[0]
    b = tap_buffers(c, n, 64, 1 << 14)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c.d.serve_spans_device(begin, n, b["rec"].data_ptr(), b["stats"].data_ptr(), b["table"].data_ptr(),
                               b["ws"].data_ptr(), b["ws"].numel() * 8, b["tap"], st.cuda_stream)
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):      # the first call of this handler's fold is the captured one
            fold_call(c, b, 64, 1 << 14, st.cuda_stream)
        for _ in range(3):
            g.replay()
    torch.cuda.synchronize()
    check_tapped(c, b, folds=3)


def test_corrupted_spans_are_refused_on_the_device(gpu):
    """Every damaged trace is refused by the read-only check phase or the vote after the replay; the device
    leaves what the host leaves."""
    c, off, spans = corruption_base()
    for name, o, bad, refused in corruptions(c, off, spans):
        s, t, w = device_fold(c, o, bad, len(o) - 1)
        hs, ht, hw = host_fold(c.h, o, bad)
        assert np.array_equal(s, hs) and np.array_equal(t, ht) and np.array_equal(w, hw), name
        check_corruption(c, o, bad, bad, refused, (s, t, w))
        invariant(c, t)         # a refused trace adds to no word but the header's count
        assert np.all(w[refused] == U64_MAX)


def test_serve_spans_with_the_critical_path(gpu):
    c, _, _ = small_whole()
    prof = isim.LoadProfile.steps([(40_000_000, 500_000), (20_000_000, 100_000)], 300_000)
    d = isim.DesHandler(c.h, profile=prof)
    begin, n = BATCHES[0]
    plain = d.serve_spans(begin, n)
    assert len(plain) == 5
    recs, stats, table, traces, waits, path = d.serve_spans(begin, n, critical_path=True)
    assert np.array_equal(recs, plain[0]) and np.array_equal(stats, plain[1]) and np.array_equal(table, plain[2])
    assert [t.trace_id for t in traces] == [t.trace_id for t in plain[3]] and np.array_equal(waits.table, plain[4].table)
    assert isinstance(path, isim.DesCriticalPath) and path.header["traces"] == len(traces) > 0
    off = np.concatenate([[0], np.cumsum([len(t) for t in traces])]).astype(np.uint64)
    hs, ht, hw = host_fold(c.h, off, np.concatenate([t.spans for t in plain[3]]))
    assert np.array_equal(np.concatenate([t.spans for t in traces]), hs)
    assert np.array_equal(path.table, ht) and np.array_equal(path.trace_wait_ns, hw)
    invariant(c, path.table)
    assert path.header["sum_latency_ns"] == sum(t.latency_ns for t in traces)
    assert traces[0].to_text().splitlines()[1].endswith(" *")
    assert len(path.to_text().splitlines()) == 2 + len(path.rows())
