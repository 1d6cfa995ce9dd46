"""Critical path on the GPU: isim_critical_path_device after
isim_trace_spans_device against isim_critical_path_host, the spans byte for
byte and the table word for word, on graphs that reach the 8-byte and the wide
nodes, u64 time, the spilling chain and every corner of the winner rule: list
lengths around the 64-entry batch, a cap one span short, a dirty workspace, a
table that starts non-zero, a captured graph replayed three times, two streams,
corrupted spans, and TraceSpans.tail_critical_path end to end in chunks."""
import numpy as np
import pytest

import isim
from isim import native
from isim.generators import config3p_topology
from isim.yamljson import obj_to_json

import critical_path_graphs as cg

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 63, 64, 65, 1000)
MODES = (isim.MODE_A, isim.MODE_B)
M64 = (1 << 64) - 1
ROW = native.CP_ROW_WORDS


def id_list(n, seed):
    """n ids around 2^32, unsorted, with repeats, and a few from the far ends of u64."""
    rng = np.random.default_rng(seed)
    ids = (np.uint64((1 << 32) - 40) + rng.integers(0, 80, n, dtype=np.uint64)).astype(np.uint64)
    if n >= 63:
        ids[5], ids[17], ids[18] = 0, (1 << 64) - 1, ids[3]
    return ids


@pytest.fixture(scope="module")
def handlers():
    return {(name, mode): cg.make(name, mode) for name in cg.CASES for mode in MODES}


def host_want(ts, ids, cap=None, table=None):
    """(offsets, spans, info, table) of the host walk and the host fold of its written traces."""
    off, spans, info = ts.raw_host(ids, cap_spans=cap)
    table = ts.fold_host(off, spans, int(info[native.SPAN_WRITTEN]), table)
    return off, spans, info, table


class DeviceCall:
    """The buffers of one isim_trace_spans_device + isim_critical_path_device pair: the workspaces filled
    with 0xFF, the span buffer with 0xEE (what the calls do not write stays that)."""

    def __init__(self, ts, ids, cap, table=None):
        import torch
        dev = torch.device("cuda", 0)
        self.ts, self.n, self.cap = ts, len(ids), cap
        self.ids = torch.from_numpy(np.ascontiguousarray(ids).view(np.int64).copy()).to(dev)
        self.off = torch.full((self.n + 1,), -1, dtype=torch.int64, device=dev)
        self.spans = torch.full((max(1, cap) * 48,), 0xEE, dtype=torch.uint8, device=dev)
        self.info = torch.full((4,), -1, dtype=torch.int64, device=dev)
        self.sws_b, self.cws_b = ts.workspace_bytes(self.n), ts.critical_path_workspace_bytes(cap)
        self.sws = torch.full((max(1, self.sws_b),), 0xFF, dtype=torch.uint8, device=dev)
        self.cws = torch.full((self.cws_b,), 0xFF, dtype=torch.uint8, device=dev)
        start = np.zeros(ts.table_words(), np.uint64) if table is None else table
        self.table = torch.from_numpy(start.view(np.int64).copy()).to(dev)

    def walk(self, stream=0):
        self.ts.spans_device(self.ids.data_ptr(), self.n, d_off=self.off.data_ptr(), d_spans=self.spans.data_ptr(),
                             cap_spans=self.cap, d_info=self.info.data_ptr(), d_workspace=self.sws.data_ptr(),
                             workspace_bytes=self.sws_b, stream=stream)

    def fold(self, stream=0):
        self.ts.critical_path_device(d_off=self.off.data_ptr(), d_spans=self.spans.data_ptr(), cap_spans=self.cap,
                                     d_info=self.info.data_ptr(), n_ids=self.n, d_table=self.table.data_ptr(),
                                     d_workspace=self.cws.data_ptr(), workspace_bytes=self.cws_b, stream=stream)

    def host(self):
        """(offsets, spans of the whole buffer, info, table) copied to the host."""
        return (self.off.cpu().numpy().view(np.uint64), self.spans.cpu().numpy().view(isim.SPAN_DTYPE)[:self.cap].copy(),
                self.info.cpu().numpy().view(np.uint64), self.table.cpu().numpy().view(np.uint64))


def check(got, want, cap):
    """The device's buffers against the host's: offsets, info, table, the written spans; the rest of the
    span buffer is as it was filled."""
    off, spans, info, table = got
    h_off, h_spans, h_info, h_table = want
    assert np.array_equal(off, h_off) and np.array_equal(info, h_info)
    end = int(h_off[int(h_info[native.SPAN_WRITTEN])])
    assert spans[:end].tobytes() == h_spans[:end].tobytes()
    assert np.all(spans[end:cap].view(np.uint8) == 0xEE)
    assert np.array_equal(table, h_table), (table.reshape(-1, ROW), h_table.reshape(-1, ROW))


@pytest.mark.parametrize("mode", MODES, ids=("modeA", "modeB"))
@pytest.mark.parametrize("name", list(cg.CASES))
def test_device_equals_host(gpu, handlers, name, mode):
    """Every list length, from a dirty workspace (0xFF)."""
    ts = isim.TraceSpans(handlers[(name, mode)])
    for n in LENGTHS:
        ids = id_list(n, n + 1)
        want = host_want(ts, ids)
        cap = int(want[0][-1])
        d = DeviceCall(ts, ids, cap)
        d.walk()
        d.fold()
        check(d.host(), want, cap)
        hdr = want[3].reshape(-1, ROW)[-1]
        assert hdr[:2].tolist() == [n, cap] and int(hdr[native.CP_H_REFUSED]) == 0
        # the synchronous entry point over host buffers: the same
        off, spans, _ = ts.raw_host(ids)
        spans["start_ns"] = 0
        table = ts.fold(off, spans, n)
        assert spans.tobytes() == want[1].tobytes() and np.array_equal(table, want[3])
    if name == "winners":
        crit = (want[1]["status"] & native.SPAN_CRITICAL) != 0
        assert crit.any() and not crit.all()


def test_cap_one_short_and_a_table_that_starts_non_zero(gpu, handlers):
    ts = isim.TraceSpans(handlers[("concurrent", isim.MODE_B)])
    ids = id_list(200, 3)
    off, _, _ = ts.raw_host(ids)
    total = int(off[-1])
    start = np.arange(ts.table_words(), dtype=np.uint64) * np.uint64(0x0123456789ABCDEF) + np.uint64(M64 - 3)
    for cap in (total - 1, int(off[100]) + 1, int(off[1]) - 1):
        want = host_want(ts, ids, cap, start.copy())
        d = DeviceCall(ts, ids, cap, start)
        d.walk()
        d.fold()
        check(d.host(), want, cap)        # the unwritten tail is untouched: 0xEE
        fit = int(np.searchsorted(off, cap, side="right")) - 1
        added = (want[3].astype(object) - start.astype(object)).reshape(-1, ROW)
        assert [int(x) & M64 for x in added[-1][:2]] == [fit, int(off[fit])]      # only the written traces


def test_captured_graph_replayed_three_times(gpu):
    """Spans and critical path captured as the handler's first use of the device: the table takes three
    adds, the spans are one run's."""
    import torch
    for name in ("winners", "chain40"):
        ts = isim.TraceSpans(cg.make(name, isim.MODE_B))       # a fresh handler: nothing uploaded yet
        ids = id_list(300, 9)
        want = host_want(ts, ids)
        cap = int(want[0][-1])
        d = DeviceCall(ts, ids, cap)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            s = torch.cuda.current_stream().cuda_stream
            d.walk(s)
            d.fold(s)
        d.table.zero_()
        for fill in (0xC3, 0x00, 0xFF):
            d.sws.fill_(fill)
            d.cws.fill_(fill)
            g.replay()
        off, spans, info, table = d.host()
        assert np.array_equal(off, want[0]) and spans.tobytes() == want[1].tobytes()
        assert table.tolist() == [(3 * int(x)) & M64 for x in want[3]]


def test_two_streams(gpu, handlers):
    """Two streams at once, several calls each, each with its own workspaces and table."""
    import torch
    ts = isim.TraceSpans(handlers[("chain40", isim.MODE_A)])
    lists = [id_list(1000, 21), id_list(1000, 22) + np.uint64(1 << 20)]
    want = [host_want(ts, ids) for ids in lists]
    calls = [DeviceCall(ts, ids, int(w[0][-1])) for ids, w in zip(lists, want)]
    streams = [torch.cuda.Stream(torch.device("cuda", 0)) for _ in lists]
    torch.cuda.synchronize()
    for _ in range(3):
        for c, s in zip(calls, streams):
            c.walk(s.cuda_stream)
            c.fold(s.cuda_stream)
    torch.cuda.synchronize()
    for c, w in zip(calls, want):
        off, spans, info, table = c.host()
        assert np.array_equal(off, w[0]) and spans.tobytes() == w[1].tobytes()
        assert table.tolist() == [(3 * int(x)) & M64 for x in w[3]]


@pytest.mark.parametrize("kind", cg.CORRUPTIONS)
def test_corrupted_spans_are_refused_on_the_device(gpu, handlers, kind):
    """Spans that are no walk's: refused, counted, nothing else written, as on the host."""
    import torch
    h = handlers[("winners", isim.MODE_B)]
    ts = isim.TraceSpans(h)
    ids = np.arange(100, 140, dtype=np.uint64)
    d = DeviceCall(ts, ids, int(ts.raw_host(ids)[0][-1]))
    d.walk()
    off, spans, info, _ = d.host()
    off = off.copy()
    refused = cg.corrupt(kind, off, spans, 17, 0xFFFFFFF0, len(ts.names))
    d.off.copy_(torch.from_numpy(off.view(np.int64)))
    d.spans.copy_(torch.from_numpy(spans.view(np.uint8)))
    d.fold()
    want_table = ts.fold_host(off, spans, len(ids))
    got = d.host()
    assert np.array_equal(got[0], off) and got[1].tobytes() == spans.tobytes()
    assert np.array_equal(got[3], want_table)
    assert int(got[3].reshape(-1, ROW)[-1, native.CP_H_REFUSED]) == len(refused)


def test_tail_critical_path_in_chunks(gpu):
    h = isim.Handler(isim.ServiceGraph.from_json(obj_to_json(config3p_topology(50, n=200))), None, isim.SimParams())
    n, begin = 20_000, (1 << 32) - 10_000
    recs, _ = h.serve(begin, n)
    ts = isim.TraceSpans(h)
    p99 = int(np.sort(recs["latency_ns"])[isim.quantile_rank(n, 990000) - 1])
    ids = (np.flatnonzero(recs["latency_ns"] >= np.uint64(p99)) + begin).astype(np.uint64)
    off, spans, info, table = host_want(ts, ids)
    lens = np.diff(off.astype(np.int64))
    cap = max(int(lens.max()), int(off[-1]) // 4)
    chunks, room = 1, cap
    for m in lens.tolist():         # the chunks of a greedy fill
        if m > room:
            chunks, room = chunks + 1, cap
        room -= m
    assert chunks >= 3
    cp = ts.tail_critical_path(recs, begin, q_ppm=990000, cap_spans=cap, keep_traces=True)
    assert np.array_equal(cp.table.reshape(-1), table)
    assert cp.header["traces"] == len(ids) and cp.header["sum_latency_ns"] == int(recs["latency_ns"][ids - begin].sum())
    assert [t.trace_id for t in cp.traces] == ids.tolist()
    assert np.concatenate([t.spans for t in cp.traces]).tobytes() == spans.tobytes()
    rows = cp.rows()
    assert sum(r["path_ns"] for r in rows) == cp.header["sum_latency_ns"]
    assert cp.to_text().count("\n") == 1 + len(rows)
    # a buffer smaller than the first trace grows to hold it
    small = ts.tail_critical_path(recs, begin, q_ppm=990000, max_traces=5, cap_spans=1)
    assert np.array_equal(small.table.reshape(-1), host_want(ts, ids[:5])[3])
