"""Trace spans on the GPU: the device walks against
isim_trace_spans_host byte for byte (spans, offsets, info) on the smallest
graphs that reach each kernel variant, list lengths around the 64-entry batch,
a cap one span short, a dirty workspace, a captured graph, two streams on the
spilling chain, the selection against numpy, and TraceSpans.slowest end to end."""
import json

import numpy as np
import pytest

import isim
from isim import native
from isim.generators import config3p_topology, tree_topology
from isim.yamljson import obj_to_json

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 63, 64, 65, 1000)


def _calls(doc):
    for s in doc["services"]:
        for st in s.get("script", []):
            for c in (st if isinstance(st, list) else [st]):
                if "call" in c:
                    yield c


def _tree(sequential, prob=None, error_rate=0.1, sleep=None):
    doc = tree_topology(3, 3, sequential=sequential)
    for s in doc["services"]:
        s["errorRate"] = error_rate
        if sleep:
            s["script"] = [{"sleep": sleep}] + list(s.get("script") or [])
    for c in _calls(doc):
        if prob:
            c["call"] = {"service": c["call"] if isinstance(c["call"], str) else c["call"]["service"], "probability": prob}
    return doc


def _chain(depth, prob=90):
    """c0 -> c1 -> ... each link also calling two leaves in one concurrent step, every call probabilistic."""
    svcs = []
    for i in range(depth):
        calls = [[{"call": {"service": n, "probability": prob}} for n in (f"c{i + 1}", f"l{i}-0", f"l{i}-1")]] \
            if i + 1 < depth else []
        svcs.append({"name": f"c{i}", "script": [{"sleep": "1us"}] + calls, "errorRate": 0.02})
        svcs += [{"name": f"l{i}-{j}", "errorRate": 0.03} for j in range(2)]
    svcs[0]["isEntrypoint"] = True
    return {"services": svcs}


D, W = native.FLAG_DYNAMIC, native.FLAG_TREE_WIDE
# name -> (graph, flags); the comment names the kernel variant the graph is there for
CASES = {
    "fanout": (_tree(True, prob=60), D),                     # a fan-out tree of depth 3, sequential steps
    "concurrent": (_tree(False, prob=60), D),                # concurrent steps
    "static-err30": (_tree(False, error_rate=0.3), D),       # a static graph on the dynamic path
    "chain12": (_chain(12), D),                              # 16 register frames
    "chain40": (_chain(40), D),                              # 8 register frames + the spill columns
    "time64": (_tree(True, prob=60, sleep="2s"), D),         # latency bound past 2^32 ns: u64 time
    "wide": (_tree(False, prob=60), D | W),                  # 16-byte nodes
    "wide-chain40": (_chain(40), D | W),                     # ... and the spill
}
MODES = (isim.MODE_A, isim.MODE_B)


def make(name, mode):
    doc, flags = CASES[name]
    return isim.Handler(isim.ServiceGraph.from_json(obj_to_json(doc)), None,
                        isim.SimParams(error_mode=mode, flags=flags))


def id_list(n, seed):
    """n ids around 2^32, unsorted, with repeats, and a few from the far ends of u64."""
    rng = np.random.default_rng(seed)
    ids = (np.uint64((1 << 32) - 40) + rng.integers(0, 80, n, dtype=np.uint64)).astype(np.uint64)
    if n >= 63:
        ids[5], ids[17], ids[18] = 0, (1 << 64) - 1, ids[3]
    return ids


@pytest.fixture(scope="module")
def handlers():
    return {(name, mode): make(name, mode) for name in CASES for mode in MODES}


def test_variants_are_reached(gpu, handlers):
    assert handlers[("time64", 0)].info.max_latency_ns >= 1 << 32
    assert handlers[("fanout", 0)].info.max_latency_ns < 1 << 32
    assert handlers[("chain40", 0)].info.max_depth == 40 and handlers[("chain12", 0)].info.max_depth == 12
    assert handlers[("wide", 0)].launch_info(0)["tree_wide"] == 1
    assert handlers[("fanout", 0)].launch_info(0)["tree_wide"] == 0


@pytest.mark.parametrize("mode", MODES, ids=("modeA", "modeB"))
@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_host(gpu, handlers, name, mode):
    ts = isim.TraceSpans(handlers[(name, mode)])
    for n in LENGTHS:
        ids = id_list(n, n + 1)
        off, spans, info = ts.raw(ids)
        h_off, h_spans, h_info = ts.raw_host(ids)
        assert np.array_equal(info, h_info) and np.array_equal(off, h_off), (name, mode, n)
        assert spans.tobytes() == h_spans.tobytes(), (name, mode, n)
        assert list(info) == [int(off[-1]), n, n, n]
    if mode == isim.MODE_B:
        st = h_spans["status"]
        assert np.any(st == 3) and np.any(st == 1)      # the lists hold own draws and failed steps


def test_cap_one_short(gpu, handlers):
    ts = isim.TraceSpans(handlers[("concurrent", isim.MODE_B)])
    ids = id_list(200, 3)
    off, spans, info = ts.raw_host(ids)
    total = int(off[-1])
    for cap in (total - 1, int(off[100]), int(off[100]) + 1, 0):
        want = ts.raw_host(ids, cap_spans=cap)
        got = ts.raw(ids, cap_spans=cap)
        fit = int(np.searchsorted(off, cap, side="right")) - 1
        assert list(got[2]) == [total, fit, 200, fit] == list(want[2]), cap
        assert np.array_equal(got[0], off) and got[1].tobytes() == want[1].tobytes()
        assert got[1][:int(off[fit])].tobytes() == spans[:int(off[fit])].tobytes()
        assert not got[1][int(off[fit]):].view(np.uint8).any()     # the trace that does not fit writes nothing


class DeviceCall:
    """The buffers of one isim_trace_spans_device call, the workspace filled with a byte."""

    def __init__(self, ts, ids, cap, fill=0xA5):
        import torch
        dev = torch.device("cuda", 0)
        self.ts, self.n, self.cap = ts, len(ids), cap
        self.ids = torch.from_numpy(np.ascontiguousarray(ids).view(np.int64).copy()).to(dev)
        self.off = torch.full((self.n + 1,), -1, dtype=torch.int64, device=dev)
        self.spans = torch.zeros(max(1, cap) * 48, dtype=torch.uint8, device=dev)
        self.info = torch.full((4,), -1, dtype=torch.int64, device=dev)
        self.wsb = ts.workspace_bytes(self.n)
        self.ws = torch.full((max(1, self.wsb),), fill, dtype=torch.uint8, device=dev)

    def call(self, stream=0):
        self.ts.spans_device(self.ids.data_ptr(), self.n, d_off=self.off.data_ptr(), d_spans=self.spans.data_ptr(),
                             cap_spans=self.cap, d_info=self.info.data_ptr(), d_workspace=self.ws.data_ptr(),
                             workspace_bytes=self.wsb, stream=stream)

    def host(self):
        off = self.off.cpu().numpy().view(np.uint64)
        info = self.info.cpu().numpy().view(np.uint64)
        spans = self.spans.cpu().numpy().view(isim.SPAN_DTYPE)[:self.cap].copy()
        assert not spans["start_ns"].any()      # the device entry point leaves the start times 0
        self.ts.place(off, spans, int(info[native.SPAN_WRITTEN]))
        return off, spans, info


def test_dirty_workspace_and_capture(gpu):
    """The call captured in a graph as the handler's first use of the device, replayed three times with the
    workspace and the outputs refilled in between: the host walk's bytes each time."""
    import torch
    for name in ("concurrent", "chain40"):
        ts = isim.TraceSpans(make(name, isim.MODE_B))      # a fresh handler: nothing uploaded yet
        ids = id_list(300, 9)
        h_off, h_spans, h_info = ts.raw_host(ids)
        d = DeviceCall(ts, ids, int(h_off[-1]))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            d.call(torch.cuda.current_stream().cuda_stream)
        for fill in (0xC3, 0x00, 0xFF):
            d.ws.fill_(fill)
            d.off.fill_(-1)
            d.info.fill_(-1)
            d.spans.zero_()
            g.replay()
            off, spans, info = d.host()
            assert np.array_equal(off, h_off) and np.array_equal(info, h_info), (name, fill)
            assert spans.tobytes() == h_spans.tobytes(), (name, fill)


def test_two_streams_on_the_spilling_chain(gpu, handlers):
    """Two streams at once, several calls each, each with its own workspace (its own spill columns)."""
    import torch
    ts = isim.TraceSpans(handlers[("chain40", isim.MODE_A)])
    lists = [id_list(1000, 21), id_list(1000, 22) + np.uint64(1 << 20)]
    want = [ts.raw_host(ids) for ids in lists]
    calls = [DeviceCall(ts, ids, int(w[0][-1])) for ids, w in zip(lists, want)]
    streams = [torch.cuda.Stream(torch.device("cuda", 0)) for _ in lists]
    torch.cuda.synchronize()
    for _ in range(4):
        for c, s in zip(calls, streams):
            c.call(s.cuda_stream)
    torch.cuda.synchronize()
    for c, w in zip(calls, want):
        off, spans, info = c.host()
        assert np.array_equal(off, w[0]) and np.array_equal(info, w[2]) and spans.tobytes() == w[1].tobytes()


@pytest.mark.parametrize("n", (8191, 8192, 8193))
def test_select_against_numpy(gpu, n):
    rng = np.random.default_rng(n)
    recs = np.zeros(n, isim.REC_DTYPE)
    recs["latency_ns"] = rng.integers(0, 1 << 40, n, dtype=np.uint64)
    recs["status_err"] = np.where(rng.random(n) < 0.2, 0x80000001, 0).astype(np.uint32)
    recs["latency_ns"][n - 1] = recs["latency_ns"].max()          # the last record of the last tile matches
    begin = (1 << 32) - 4000
    lat = recs["latency_ns"]
    for thr in (int(lat.max()) + 1, 0, int(np.sort(lat)[n - n // 100])):      # none, all, about 1 %
        for cls in (native.Q_ALL, native.Q_200, native.Q_500):
            m = lat >= np.uint64(thr)
            if cls != native.Q_ALL:
                m &= (recs["status_err"] >> 31) == (1 if cls == native.Q_500 else 0)
            want = np.flatnonzero(m).astype(np.uint64) + np.uint64(begin)
            ids, matches = isim.select_traces(recs, begin, thr, cls)
            assert matches == len(want) and np.array_equal(ids, want), (thr, cls)      # ascending
            ids, matches = isim.select_traces(recs, begin, thr, cls, max_ids=7)
            assert matches == len(want) and np.array_equal(ids, want[:7])
    ids, matches = isim.select_traces(recs[:0], begin, 0)
    assert matches == 0 and len(ids) == 0


def test_slowest_end_to_end(gpu):
    h = isim.Handler(isim.ServiceGraph.from_json(obj_to_json(config3p_topology(50, n=200))), None, isim.SimParams())
    n, begin = 20_000, (1 << 32) - 10_000
    recs, _ = h.serve(begin, n)
    ts = isim.TraceSpans(h)
    traces = ts.slowest(recs, begin)
    p999 = int(np.sort(recs["latency_ns"])[isim.quantile_rank(n, 999000) - 1])
    want_ids = (np.flatnonzero(recs["latency_ns"] >= np.uint64(p999)) + begin)[:64]
    assert 1 <= len(traces) <= 64 and [t.trace_id for t in traces] == want_ids.tolist()
    host = ts.spans_host(want_ids)
    for t, w in zip(traces, host):
        r = recs[t.trace_id - begin]
        assert t.latency_ns >= p999 and t.latency_ns == int(r["latency_ns"]) and len(t) == int(r["hops"])
        assert t.spans.tobytes() == w.spans.tobytes()
        assert t.to_text().count("\n") == len(t)
