"""Per-service percentiles on the GPU: isim_service_quantiles_device against
isim_service_quantiles_host, word for word with the header, on synthetic spans uploaded as one list entry
(span counts around a wave, one service for every lane, segments around the LDS stage, long segments that
end inside a chunk or follow each other, long and short and empty services interleaved, top bytes that
differ by measure, ties, 16 quantiles, corrupted spans); a dirty workspace and table, two streams, a
captured graph; and DesHandler.service_quantiles against the wait table, the DES table and
isim.latency_quantiles of the same batch."""
import numpy as np
import pytest

import isim
from isim import native
from isim.service_quantiles import (CHUNK, STAGE, service_quantiles_device, service_quantiles_table_words,
                                    service_quantiles_workspace_bytes)

from test_des_gpu import DesCase
from test_des_spans_gpu import run_tap
from test_service_quantiles import services

pytestmark = pytest.mark.gpu

Q3 = (0.5, 0.99, 1.0)
Q16 = (0.0, 0.000001, 0.01, 0.05, 0.1, 0.25, 0.4, 0.5, 0.6, 0.75, 0.9, 0.95, 0.99, 0.999, 0.999999, 1.0)
M64 = (1 << 64) - 1


def spread(rng, n):
    """Waits over many magnitudes, services around 2^20: the digits at which quantiles part differ."""
    wait = (rng.integers(0, 1 << 62, n, dtype=np.uint64) >> rng.integers(0, 62, n).astype(np.uint64))
    return wait, rng.integers(0, 1 << 20, n, dtype=np.uint64)


def synth(lengths, seed=1, values=spread, p500=0.3):
    """Spans of len(lengths) services, lengths[s] of service s, shuffled: a random arrival below 2^40,
    (wait, service) from values(rng, n), status bit 0 set with probability p500 (bit 1 is noise)."""
    rng = np.random.default_rng(seed)
    n = int(sum(lengths))
    out = np.zeros(n, isim.DES_SPAN_DTYPE)
    out["service"] = rng.permutation(np.repeat(np.arange(len(lengths), dtype=np.uint32), lengths))
    wait, service = values(rng, n)
    out["arrival_ns"] = rng.integers(0, 1 << 40, n, dtype=np.uint64)
    out["start_ns"] = out["arrival_ns"] + wait
    out["finish_ns"] = out["start_ns"] + service
    out["status"] = (rng.random(n) < p500).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 1)
    return out


def device_table(h, spans, q, cap_spans=None, written_spans=None, stream=None):
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
    words = service_quantiles_table_words(h, len(q))
    d_out = torch.full((words,), -1, dtype=torch.int64, device=dev)
    ws_bytes = service_quantiles_workspace_bytes(h, cap, len(q))
    ws = torch.full((max(8, ws_bytes),), 0xFF, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    service_quantiles_device(h, q, d_off.data_ptr(), d_spans.data_ptr(), cap, d_info.data_ptr(), d_out.data_ptr(),
                             ws.data_ptr(), ws_bytes, s)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint64)


def same_as_host(h, spans, q, **kw):
    got = device_table(h, spans, q, **kw)
    want = isim.service_quantiles_host(h, spans, q)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:6], got[bad[:6]], want[bad[:6]])
    return got


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_span_counts(gpu, n):
    h = services(3)
    spans = synth([n // 3, n - n // 3 - n // 4, n // 4], seed=n)
    t = same_as_host(h, spans, Q3)
    assert list(t[-2:]) == [n, 0]
    # cap_spans only bounds the grids and the count: a longer buffer of which n spans were written, a list
    # that claims more than the buffer holds, and cap_spans 0
    if n == 65:
        more = synth([40, 50, 45], seed=3)
        assert np.array_equal(device_table(h, more, Q3, written_spans=n), isim.service_quantiles_host(h, more[:n], Q3))
        assert np.array_equal(device_table(h, more[:n], Q3, written_spans=n + 70), isim.service_quantiles_host(h, more[:n], Q3))
        assert not device_table(h, more, Q3, cap_spans=0).any()


@pytest.mark.parametrize("n", [2000, STAGE + 500], ids=["short", "long"])
def test_one_service_holds_every_span(gpu, n):
    t = same_as_host(services(1), synth([n], seed=5), Q3)
    assert int(t[0]) == n


@pytest.mark.parametrize("n", [STAGE - 1, STAGE, STAGE + 1])
def test_segments_around_the_stage(gpu, n):
    t = same_as_host(services(3), synth([10, n, 70], seed=n), Q16)
    assert int(t[9 * 17]) == n      # the ALL count of service 1


LONG = {
    "ends_inside_a_chunk": [2 * CHUNK + 777],
    "a_whole_number_of_chunks": [2 * CHUNK, 5],
    "two_meet_inside_a_chunk": [STAGE + 100, CHUNK + 50],
    "interleaved": [0, CHUNK + 904, 0, 17, 2 * CHUNK + 808, 0, 0, STAGE, CHUNK + 1, 1, 0],
}


@pytest.mark.parametrize("name", list(LONG))
def test_long_segments(gpu, name):
    lengths = LONG[name]
    t = same_as_host(services(len(lengths)), synth(lengths, seed=7), Q3)
    cells, hdr = isim.decode_service_quantiles(t, len(lengths), len(Q3))
    assert list(cells[:, 0, 0, 0]) == lengths and hdr == {"folded": sum(lengths), "refused": 0}


def by_measure(rng, n):
    """A third each: wait below 2^8 with a service time around 2^40; wait at or above 2^56 with a service time
    below 2^16; all zero.  The top byte, and so the digit passes that are skipped, differ by measure."""
    kind = rng.integers(0, 3, n)
    wait = np.where(kind == 0, rng.integers(0, 1 << 8, n, dtype=np.uint64),
                    np.where(kind == 1, rng.integers(1 << 56, 1 << 62, n, dtype=np.uint64), np.uint64(0)))
    service = np.where(kind == 0, rng.integers(1 << 40, 1 << 41, n, dtype=np.uint64),
                       np.where(kind == 1, rng.integers(0, 1 << 16, n, dtype=np.uint64), np.uint64(0)))
    return wait.astype(np.uint64), service.astype(np.uint64)


def one_kind(kind):
    def values(rng, n):
        z = np.zeros(n, np.uint64)
        if kind == 2:
            return z, z
        lo, hi = ((0, 1 << 8), (1 << 40, 1 << 41)) if kind == 0 else ((1 << 56, 1 << 62), (0, 1 << 16))
        return rng.integers(*lo, n, dtype=np.uint64), rng.integers(*hi, n, dtype=np.uint64)
    return values


def test_top_bytes_differ_by_measure(gpu):
    h = services(4)
    lengths = [CHUNK + 300, 900, STAGE + 1, 40]
    # every service mixes the three kinds; then each service is of one kind, a long and a short one all zero
    same_as_host(h, synth(lengths, seed=11, values=by_measure), Q16)
    parts = [synth([0] * s + [lengths[s]], seed=20 + s, values=one_kind(k)) for s, k in enumerate([0, 1, 2, 2])]
    t = same_as_host(h, np.concatenate(parts), Q3)
    cells, _ = isim.decode_service_quantiles(t, 4, len(Q3))
    assert int(cells[0, 0, 0, 3]) < 1 << 8 and int(cells[0, 1, 0, 1]) >= 1 << 40 and int(cells[1, 2, 0, 1]) >= 1 << 56
    assert not cells[2:, :, :, 1:].any() and list(cells[2:, 0, 0, 0]) == lengths[2:]


def ties(rng, n):
    pick = np.array([0, 1, 1 << 32, M64 >> 1], np.uint64)
    return pick[rng.integers(0, 4, n)], pick[rng.integers(0, 3, n)]


def test_heavy_ties_and_the_extremes(gpu):
    h = services(3)
    spans = synth([CHUNK + 11, 700, 64], seed=13, values=ties)
    spans[:4]["arrival_ns"], spans[:4]["start_ns"], spans[:4]["finish_ns"] = 0, [0, M64, 0, M64], [0, M64, M64, M64]
    same_as_host(h, spans, Q16)
    same_as_host(h, spans, (0.5,))


def test_sixteen_quantiles_part_at_different_digits(gpu):
    h = services(2)
    spans = synth([3 * CHUNK + 5, STAGE - 7], seed=17, p500=0.5)
    t = same_as_host(h, spans, Q16)
    cells, _ = isim.decode_service_quantiles(t, 2, 16)
    for s in range(2):
        v = [int(x) for x in cells[s, 0, 0, 1:]]
        assert v == sorted(v) and len({x.bit_length() // 8 for x in v}) >= 4     # they part at four digits at least
    # the same through the synchronous entry point
    assert np.array_equal(isim.service_quantiles(h, spans, Q16), t)


def test_corrupted_spans_are_refused_as_on_the_host(gpu):
    h = services(5)
    spans = synth([CHUNK + 100, 300, 0, 2000, 77], seed=19)
    m = len(spans)
    bad = spans.copy()
    pick = np.random.default_rng(5).permutation(m)
    bad["service"][pick[:100]] = 5
    bad["service"][pick[100:200]] = 0xFFFFFFFF
    bad["start_ns"][pick[200:300]] = bad["arrival_ns"][pick[200:300]] - 1
    bad["finish_ns"][pick[300:400]] = bad["start_ns"][pick[300:400]] - 1
    bad["start_ns"][pick[400:450]] = M64
    t = same_as_host(h, bad, Q3)
    assert int(t[-2 + native.SVQ_H_REFUSED]) >= 400 and int(t[-2]) + int(t[-1]) == m
    keep = np.ones(m, bool)
    keep[pick[:450]] = False
    assert np.array_equal(t[:-2], isim.service_quantiles_host(h, bad[keep], Q3)[:-2])   # a refused span adds to nothing else


class Buffers:
    """The device buffers of one call over uploaded spans, workspace and table dirty."""

    def __init__(self, h, spans, q, fill):
        import torch
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).ravel().copy()).to("cuda")  # noqa: E731
        self.h, self.q, self.n = h, q, len(spans)
        self.spans, self.off = up(spans), up(np.array([0, len(spans)], np.uint64))
        self.info = up(np.array([len(spans), 1, 1, 1, 1], np.uint64))
        self.words = service_quantiles_table_words(h, len(q))
        self.out = torch.full((self.words,), fill, dtype=torch.int64, device="cuda")
        self.ws_bytes = service_quantiles_workspace_bytes(h, len(spans), len(q))
        self.ws = torch.full((self.ws_bytes // 8 + 1,), fill, dtype=torch.int64, device="cuda")

    def call(self, stream):
        service_quantiles_device(self.h, self.q, self.off.data_ptr(), self.spans.data_ptr(), self.n, self.info.data_ptr(),
                                 self.out.data_ptr(), self.ws.data_ptr(), self.ws_bytes, stream)

    def table(self):
        return self.out.cpu().numpy().view(np.uint64)


MIXED = [CHUNK + 904, 0, 17, STAGE + 1, 600]


def test_two_calls_on_two_streams(gpu):
    import torch
    h = services(len(MIXED))
    spans = [synth(MIXED, seed=23), synth(MIXED[::-1], seed=29)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    bufs = [Buffers(h, s, Q3, fill) for s, fill in zip(spans, (-1, 0x0101010101010101))]
    torch.cuda.synchronize()
    for st, b in zip(streams, bufs):
        with torch.cuda.stream(st):
            b.call(st.cuda_stream)
            b.call(st.cuda_stream)      # again over the workspace the first call left
    torch.cuda.synchronize()
    for s, b in zip(spans, bufs):
        assert np.array_equal(b.table(), isim.service_quantiles_host(h, s, Q3))


def test_the_call_captured_in_a_graph(gpu):
    import torch
    h = services(len(MIXED))
    spans = synth(MIXED, seed=31)
    b = Buffers(h, spans, Q16, -1)
    want = isim.service_quantiles_host(h, spans, Q16)
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


def tree(levels, branches, replicas=1, error_rate=0.0):
    """A concurrent tree, 1 ms of sleep in every service before its calls."""
    from isim.generators import tree_topology
    t = tree_topology(levels, branches, num_replicas=replicas)
    for s in t["services"]:
        s["errorRate"] = error_rate
        s["script"] = [{"sleep": "1ms"}] + s.get("script", [])
    return t


E2E = {
    "overloaded_tree": dict(doc=lambda: tree(3, 3), mean=700_000, n=3000),                       # 13 services
    "replicas_and_500s": dict(doc=lambda: tree(3, 2, replicas=3, error_rate=0.1), mean=300_000, n=3000),
}


@pytest.mark.parametrize("name", list(E2E))
def test_handler_service_quantiles(gpu, name):
    e = E2E[name]
    c = DesCase(e["doc"](), e["mean"], flags=native.FLAG_DYNAMIC)
    begin, n = 1000, e["n"]
    ns = c.h.info.n_services
    q = Q3
    sq = c.d.service_quantiles(begin, n, q)
    assert isinstance(sq, isim.ServiceQuantiles) and sq.header["refused"] == 0
    # the same batch tapped by hand: its spans, wait table, DES table and records
    r = run_tap(c, begin, n, cap_spans=n * int(c.h.info.hops_upper))
    total = int(r["off"][n])
    spans = r["spans"][:total]
    assert sq.header["folded"] == total
    assert np.array_equal(sq.flat, isim.service_quantiles_host(c.h, spans, q))
    wt, des = r["wait"], c.d.fold(r["table"])
    assert int((spans["start_ns"] > spans["arrival_ns"]).sum()) > 0    # contended
    assert np.array_equal(sq.counts["all"], wt[:ns, native.DW_INVOCATIONS])
    assert np.array_equal(sq.counts["all"], des[:, native.DES_COUNT])
    assert np.array_equal(sq.counts["500"], wt[:ns, native.DW_RESP_500])
    assert np.array_equal(sq.counts["200"], wt[:ns, native.DW_INVOCATIONS] - wt[:ns, native.DW_RESP_500])
    assert np.array_equal(sq.values["wait"]["all"][:, q.index(1.0)], wt[:ns, native.DW_MAX_WAIT])
    # the entry is invoked by the client only: its durations are the records' latencies
    entry = int(spans["service"][0])
    assert not np.any((spans["service"] == entry) & (spans["hop"] != 0))
    lq = isim.latency_quantiles(r["recs"], q)
    for cls in ("all", "200", "500"):
        assert int(sq.counts[cls][entry]) == lq[cls]["count"]
        assert [int(x) for x in sq.values["duration"][cls][entry]] == [lq[cls]["q"][f] for f in q]
    if name == "replicas_and_500s":
        assert int(sq.counts["500"].sum()) > 0
    assert len(sq.to_text(top=3).splitlines()) == 5 and len(sq.worst("wait", 0.99, 2)) == 2
    # with workers to spare nobody waits: every WAIT word past the count is 0
    pooled = isim.DesHandler(c.h, e["mean"])
    try:
        pooled.workers = 4096
        free = pooled.service_quantiles(begin, n, q)
        assert not free.cells[:, native.SVQ_WAIT, :, 1:].any() and int(free.counts["all"].sum()) > 0
        # a cap that is too small raises: never a partial table
        with pytest.raises(RuntimeError):
            pooled.service_quantiles(begin, n, q, cap_spans=int(free.header["folded"]) - 1)
    finally:
        pooled.workers = None
