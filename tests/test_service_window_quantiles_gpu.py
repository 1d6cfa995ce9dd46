"""Per-service percentiles over time on the GPU: isim_service_window_quantiles_device against
isim_service_window_quantiles_host, word for word with the header, over a 0xFF workspace and a 0xFF table, on
synthetic spans uploaded as one list entry (span counts around a wave, cap_spans on either side of what was
written, cells around the wave tier and around the LDS stage, class splits of a wave-tier cell, long cells
that end inside a chunk or follow each other, all four kinds of cell in one service's rows, finishes on the
rows' edges, windows of 1 ns and windows whose end is past 2^64, a table whose scan crosses its tile, ties, 16
quantiles and one, top bytes that differ by measure, corrupted spans); two streams, a captured graph; and
DesHandler.service_window_quantiles against the host's table, the service timeline and
isim.timeline_quantiles of the same batch."""
import numpy as np
import pytest

import isim
from isim import native
from isim.service_quantiles import CHUNK, STAGE
from isim.service_window_quantiles import (WAVE, service_window_quantiles_device, service_window_quantiles_host,
                                           service_window_quantiles_table_words,
                                           service_window_quantiles_workspace_bytes)

from test_des_gpu import DesCase
from test_des_spans_gpu import run_tap
from test_service_quantiles import services
from test_service_quantiles_gpu import E2E, Q3, Q16, by_measure, spread, ties

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
T0, W = 1 << 40, 1 << 30      # the windows of synth(): row 0 ends at 2^40, each window is 2^30 ns


def synth(lengths, seed=1, values=spread, p500=0.3):
    """Spans of len(lengths) services, lengths[s][r] of them finishing in row r (windows (T0, W,
    len(lengths[s]) - 2)), shuffled: the finish anywhere in the row, (wait, service) from values(rng, n) cut to
    what the finish leaves, status bit 0 set with probability p500 (bit 1 is noise)."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, np.int64)
    ns, rows = lengths.shape
    n = int(lengths.sum())
    out = np.zeros(n, isim.DES_SPAN_DTYPE)
    cell = rng.permutation(np.repeat(np.arange(ns * rows), lengths.ravel()))
    row = cell % rows
    lo = np.where(row == 0, 1 << 39, T0 + (np.maximum(row, 1) - 1).astype(np.uint64) * np.uint64(W)).astype(np.uint64)
    hi = np.where(row == 0, T0, np.where(row == rows - 1, 1 << 63, lo + np.uint64(W))).astype(np.uint64)
    f = lo + (rng.integers(0, 1 << 62, n, dtype=np.uint64) % (hi - lo))
    wait, service = values(rng, n)
    service = np.minimum(service, f)
    wait = np.minimum(wait, f - service)
    out["service"] = (cell // rows).astype(np.uint32)
    out["finish_ns"], out["start_ns"], out["arrival_ns"] = f, f - service, f - service - wait
    out["status"] = (rng.random(n) < p500).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 1)
    return out


def device_table(h, spans, q, window, nw, t0, cap_spans=None, written_spans=None):
    """Uploads the spans as one list entry, selects on the current stream over a 0xFF workspace into a 0xFF
    table and returns the flat table."""
    import torch
    dev = "cuda"
    cap = len(spans) if cap_spans is None else cap_spans
    end = len(spans) if written_spans is None else written_spans
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).ravel().copy()).to(dev)  # noqa: E731
    d_spans = up(spans) if len(spans) else torch.zeros(8, dtype=torch.int64, device=dev)
    d_off = up(np.array([0, end], np.uint64))
    d_info = up(np.array([end, 1, 1, 1, 1], np.uint64))
    words = service_window_quantiles_table_words(h, len(q), window, nw, t0)
    d_out = torch.full((words,), -1, dtype=torch.int64, device=dev)
    ws_bytes = service_window_quantiles_workspace_bytes(h, cap, len(q), window, nw, t0)
    ws = torch.full((max(8, ws_bytes),), 0xFF, dtype=torch.uint8, device=dev)
    service_window_quantiles_device(h, q, window, nw, t0, d_off.data_ptr(), d_spans.data_ptr(), cap, d_info.data_ptr(),
                                    d_out.data_ptr(), ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint64)


def same_as_host(h, spans, q, window=W, nw=None, t0=T0, **kw):
    got = device_table(h, spans, q, window, nw, t0, **kw)
    want = service_window_quantiles_host(h, spans, q, window, nw, t0)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:6], got[bad[:6]], want[bad[:6]])
    return got


def counts(t, ns, nw, n_q):
    return isim.decode_service_window_quantiles(t, ns, nw, n_q)[0][:, :, 0, 0, 0]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_span_counts(gpu, n):
    h = services(3)
    a, b = n // 3, n // 4
    spans = synth([[a, 0, 0, 0], [0, n - a - b, 0, 0], [0, 0, b // 2, b - b // 2]], seed=n)
    t = same_as_host(h, spans, Q3, nw=2)
    assert list(t[-2:]) == [n, 0]
    # cap_spans only bounds the grids and the count: a longer buffer of which n spans were written, a list
    # that claims more than the buffer holds, and cap_spans 0
    if n == 65:
        more = synth([[40, 0, 9, 1], [0, 50, 0, 0], [5, 5, 5, 30]], seed=3)
        want = service_window_quantiles_host(h, more[:n], Q3, W, 2, T0)
        assert np.array_equal(device_table(h, more, Q3, W, 2, T0, written_spans=n), want)
        assert np.array_equal(device_table(h, more[:n], Q3, W, 2, T0, written_spans=n + 70), want)
        assert not device_table(h, more, Q3, W, 2, T0, cap_spans=0).any()


@pytest.mark.parametrize("n", [WAVE - 1, WAVE, WAVE + 1])
def test_cells_around_the_wave_tier(gpu, n):
    t = same_as_host(services(2), synth([[10, n, 70], [n, 0, 65]], seed=n), Q16, nw=1)
    assert counts(t, 2, 1, 16).tolist() == [[10, n, 70], [n, 0, 65]]


@pytest.mark.parametrize("p500", [0.0, 1.0, "one", 0.5], ids=["no_500", "all_500", "one_500", "even"])
def test_class_splits_of_a_wave_tier_cell(gpu, p500):
    spans = synth([[WAVE - 3, 64, 65]], seed=41, p500=0.5 if p500 == "one" else p500)
    if p500 == "one":
        for r in range(3):      # one 500 per cell, the rest 200s; then the other way round
            idx = np.flatnonzero(spans["finish_ns"] >= T0 + (r - 1) * W if r else spans["finish_ns"] < T0)
            idx = idx[spans["finish_ns"][idx] < T0 + r * W] if r < 2 else idx
            spans["status"][idx] = 0
            spans["status"][idx[0]] = 1
    t = same_as_host(services(1), spans, Q16, nw=1)
    cells, _ = isim.decode_service_window_quantiles(t, 1, 1, 16)
    assert cells[0, :, 0, 0, 0].tolist() == [WAVE - 3, 64, 65]
    if p500 == "one":
        assert cells[0, :, 0, 2, 0].tolist() == [1, 1, 1]
        spans["status"] ^= 1
        same_as_host(services(1), spans, Q3, nw=1)


@pytest.mark.parametrize("n", [STAGE - 1, STAGE, STAGE + 1])
def test_cells_around_the_stage(gpu, n):
    t = same_as_host(services(2), synth([[10, n, 0, 70], [0, 0, WAVE + 9, 0]], seed=n), Q16, nw=2)
    assert int(counts(t, 2, 2, 16)[0, 1]) == n


LONG = {
    "ends_inside_a_chunk": [[2 * CHUNK + 777, 0, 3]],
    "adjacent_cells": [[0, STAGE + 100, CHUNK + 50, 2 * CHUNK, 5]],
    # empty, wave, LDS and long cells within one service's rows, and the next service starting long
    "interleaved": [[0, CHUNK + 904, 0, 17, 2 * CHUNK + 808, WAVE + 1, 0, STAGE, CHUNK + 1, 1, 0, WAVE],
                    [STAGE + 1, 0, 0, 300, 0, 0, 64, 0, 0, 0, 2, 0]],
}


@pytest.mark.parametrize("name", list(LONG))
def test_long_cells(gpu, name):
    lengths = LONG[name]
    ns, nw = len(lengths), len(lengths[0]) - 2
    t = same_as_host(services(ns), synth(lengths, seed=7), Q3, nw=nw)
    assert counts(t, ns, nw, 3).tolist() == lengths and list(t[-2:]) == [int(np.sum(lengths)), 0]


def test_finishes_on_the_rows_edges(gpu):
    h = services(2)
    fs = [0, 99, 100, 109, 110, 119, 120, 129, 130, 131, 1 << 40, M64 - 1, M64]
    spans = np.zeros(2 * len(fs), isim.DES_SPAN_DTYPE)
    spans["finish_ns"] = fs + fs
    spans["start_ns"] = spans["finish_ns"] // np.uint64(2)
    spans["service"][len(fs):] = 1
    spans["status"] = np.arange(len(spans)) % 3 == 0
    t = same_as_host(h, spans, Q3, window=10, nw=3, t0=100)
    assert counts(t, 2, 3, 3).tolist() == [[2, 2, 2, 2, 5]] * 2
    # a window of 1 ns; one window; windows whose end t0 + n_windows * W is past 2^64; t0 past every finish but one
    for window, nw, t0 in [(1, 30, 100), (1, 1, 0), (25, 1, 100), (1 << 63, 7, 1 << 62), (M64, 65536, 120),
                           ((1 << 61) + 1, 9, M64 - 1), (3, 4, M64)]:
        same_as_host(h, spans, Q3, window=window, nw=nw, t0=t0)


def test_a_sparse_table_crosses_the_scans_tile(gpu):
    """300 services x 62 rows are 18,600 cells, more than the 8,192 of a scan tile; 20,000 spans leave most
    cells empty, a few in every tier."""
    rng = np.random.default_rng(43)
    lengths = np.zeros((300, 62), np.int64)
    hot = [(0, 0, WAVE + 40), (150, 31, STAGE + 9), (299, 61, WAVE), (8191 // 62, 8191 % 62, 200), (8192 // 62, 8192 % 62, 90)]
    for s, r, n in hot:
        lengths[s, r] = n
    rest = 20_000 - int(lengths.sum())
    np.add.at(lengths.ravel(), rng.integers(0, 300 * 62, rest // 4), 4)
    lengths[299, 0] += 20_000 - int(lengths.sum())
    t = same_as_host(services(300), synth(lengths, seed=47), Q3, nw=60)
    c = counts(t, 300, 60, 3)
    assert np.array_equal(c, lengths) and int((c == 0).sum()) > 300 * 62 // 2 and list(t[-2:]) == [20_000, 0]


def test_heavy_ties_and_the_extremes(gpu):
    h = services(2)
    spans = synth([[CHUNK + 11, 700, 64, WAVE], [3, WAVE + 1, 0, 9]], seed=13, values=ties)
    zero = np.flatnonzero(spans["service"] == 1)[:6]
    spans["arrival_ns"][zero], spans["start_ns"][zero] = 0, [0, 0, 0, M64, M64, M64]
    spans["finish_ns"][zero] = [0, 0, M64, M64, M64, M64]       # 0 and 2^64 - 1 in every measure
    same_as_host(h, spans, Q16, nw=2)
    same_as_host(h, spans, (0.5,), nw=2)


def test_sixteen_quantiles_part_at_different_digits(gpu):
    h = services(2)
    lengths = [[3 * CHUNK + 5, WAVE - 7, 0], [STAGE - 7, 40, 1]]
    spans = synth(lengths, seed=17, p500=0.5)
    t = same_as_host(h, spans, Q16, nw=1)
    cells, _ = isim.decode_service_window_quantiles(t, 2, 1, 16)
    for s, r in ((0, 0), (0, 1), (1, 0)):
        v = [int(x) for x in cells[s, r, 0, 0, 1:]]
        assert v == sorted(v) and len({x.bit_length() // 8 for x in v}) >= 4     # they part at four digits at least
    # the same through the synchronous entry point
    assert np.array_equal(isim.service_window_quantiles(h, spans, Q16, W, 1, T0), t)


def test_top_bytes_differ_by_measure(gpu):
    lengths = [[CHUNK + 300, 90], [900, WAVE], [STAGE + 1, 0], [40, 400]]
    t = same_as_host(services(4), synth(np.pad(lengths, ((0, 0), (1, 0))), seed=11, values=by_measure), Q16, nw=1)
    assert counts(t, 4, 1, 16)[:, 1:].tolist() == lengths


def test_corrupted_spans_are_refused_as_on_the_host(gpu):
    h = services(3)
    spans = synth([[CHUNK + 100, 300, 0, 50], [0, 2000, 77, WAVE + 5], [60, 60, 60, 60]], seed=19)
    m = len(spans)
    bad = spans.copy()
    pick = np.random.default_rng(5).permutation(m)
    bad["service"][pick[:100]] = 3
    bad["service"][pick[100:200]] = 0xFFFFFFFF
    bad["start_ns"][pick[200:300]] = bad["arrival_ns"][pick[200:300]] - 1
    bad["finish_ns"][pick[300:400]] = bad["start_ns"][pick[300:400]] - 1
    bad["start_ns"][pick[400:450]] = M64
    t = same_as_host(h, bad, Q3, nw=2)
    assert int(t[-2 + native.SVQ_H_REFUSED]) >= 400 and int(t[-2]) + int(t[-1]) == m
    keep = np.ones(m, bool)
    keep[pick[:450]] = False
    # a refused span adds to nothing else
    assert np.array_equal(t[:-2], service_window_quantiles_host(h, bad[keep], Q3, W, 2, T0)[:-2])


class Buffers:
    """The device buffers of one call over uploaded spans, workspace and table dirty."""

    def __init__(self, h, spans, q, nw, fill):
        import torch
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).ravel().copy()).to("cuda")  # noqa: E731
        self.h, self.q, self.n, self.nw = h, q, len(spans), nw
        self.spans, self.off = up(spans), up(np.array([0, len(spans)], np.uint64))
        self.info = up(np.array([len(spans), 1, 1, 1, 1], np.uint64))
        self.words = service_window_quantiles_table_words(h, len(q), W, nw, T0)
        self.out = torch.full((self.words,), fill, dtype=torch.int64, device="cuda")
        self.ws_bytes = service_window_quantiles_workspace_bytes(h, len(spans), len(q), W, nw, T0)
        self.ws = torch.full((self.ws_bytes // 8 + 1,), fill, dtype=torch.int64, device="cuda")

    def call(self, stream):
        service_window_quantiles_device(self.h, self.q, W, self.nw, T0, self.off.data_ptr(), self.spans.data_ptr(),
                                        self.n, self.info.data_ptr(), self.out.data_ptr(), self.ws.data_ptr(),
                                        self.ws_bytes, stream)

    def table(self):
        return self.out.cpu().numpy().view(np.uint64)


MIXED = [[CHUNK + 904, 0, 17, STAGE + 1], [600, WAVE + 1, WAVE, 0]]


def test_two_calls_on_two_streams(gpu):
    import torch
    h = services(2)
    spans = [synth(MIXED, seed=23), synth([r[::-1] for r in MIXED], seed=29)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    bufs = [Buffers(h, s, Q3, 2, fill) for s, fill in zip(spans, (-1, 0x0101010101010101))]
    torch.cuda.synchronize()
    for st, b in zip(streams, bufs):
        with torch.cuda.stream(st):
            b.call(st.cuda_stream)
            b.call(st.cuda_stream)      # again over the workspace the first call left
    torch.cuda.synchronize()
    for s, b in zip(spans, bufs):
        assert np.array_equal(b.table(), service_window_quantiles_host(h, s, Q3, W, 2, T0))


def test_the_call_captured_in_a_graph(gpu):
    import torch
    h = services(2)
    spans = synth(MIXED, seed=31)
    b = Buffers(h, spans, Q16, 2, -1)
    want = service_window_quantiles_host(h, spans, Q16, W, 2, T0)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            b.call(st.cuda_stream)      # the first call of this process with these arguments
        for _ in range(3):
            g.replay()
            st.synchronize()
            assert np.array_equal(b.table(), want)
            b.out.fill_(7)      # dirty again before the next replay
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", list(E2E))
def test_handler_service_window_quantiles(gpu, name):
    e = E2E[name]
    c = DesCase(e["doc"](), e["mean"], flags=native.FLAG_DYNAMIC)
    begin, n = 1000, e["n"]
    q = Q3
    # the batch's arrivals span about n * mean: 40 windows over most of it, the tail in "after"
    t0, nw = 1_000_000, 40
    window = n * e["mean"] // 50
    wq = c.d.service_window_quantiles(begin, n, q, window_ns=window, n_windows=nw, t0_ns=t0)
    assert isinstance(wq, isim.ServiceWindowQuantiles) and wq.header["refused"] == 0
    # the same batch tapped by hand: its spans and records
    r = run_tap(c, begin, n, cap_spans=n * int(c.h.info.hops_upper))
    total = int(r["off"][n])
    spans = r["spans"][:total]
    assert wq.header["folded"] == total
    assert np.array_equal(wq.flat, service_window_quantiles_host(c.h, spans, q, window, nw, t0))
    assert int((wq.counts["all"] > 0).sum(axis=1).min()) > 10           # every service finishes spans in many rows
    st = c.d.service_timeline(begin, n, window, nw, t0)
    rows = st.flat[:-native.SVT_ROW_WORDS].reshape(wq.counts["all"].shape + (native.SVT_ROW_WORDS,))
    assert np.array_equal(wq.counts["200"], rows[:, :, native.SVT_FINISHED])
    assert np.array_equal(wq.counts["500"], rows[:, :, native.SVT_FINISHED + 1])
    # the entry is invoked by the client only, a = A_t and F - a the latency: its durations are the
    # per-window latency percentiles of the batch's records over its DES arrivals
    entry = int(spans["service"][0])
    assert not np.any((spans["service"] == entry) & (spans["hop"] != 0))
    tq = isim.timeline_quantiles_table(c.d.arrivals(begin, n), r["recs"], window, nw, t0, q).reshape(nw + 2, 3, 1 + len(q))
    for k, cls in enumerate(("all", "200", "500")):
        assert np.array_equal(wq.cells[entry, :, native.SVQ_DURATION, k, :], tq[:, k, :]), cls
    assert len(wq.to_text(top=3).splitlines()) == 5 and len(wq.worst("wait", 0.99, 2)) == 2
    assert wq.series(entry, "duration", 1.0).shape == (nw + 2,)
    # a cap one span too small raises: never a partial table
    with pytest.raises(RuntimeError):
        c.d.service_window_quantiles(begin, n, q, window_ns=window, n_windows=nw, t0_ns=t0, cap_spans=total - 1)
