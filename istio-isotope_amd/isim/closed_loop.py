"""Closed-loop clients: connection-limited arrivals for every walk.

    c = isim.ClosedLoop(connections=64)                      # qps "max", the reference's client
    c = isim.ClosedLoop(connections=64, qps=1000)            # paced: no request before its slot
    recs, _ = handler.serve(0, n)
    a, free_at, info = c.arrivals(recs)                      # u64 arrivals, the connections' state, totals
    isim.timeline(a, recs, window_ns=10**9, n_windows=60)    # the whole reporting stack takes them
    r = isim.ClosedLoopRun(handler, c, duration_ns=5 * 10**9, window_ns=10**8).run()

Each of C connections sends its next request when the previous response has
arrived and, when paced, not before its slot: for a walk, whose latencies do
not depend on when a trace starts, an exact integer recurrence over the
records, in libisim (isim_closed_loop_host on the host, isim_closed_loop* on
the GPU).  Batches with consecutive ``first_index`` that pass ``free_at`` along
equal one big batch.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import native
from .sim import REC_DTYPE
from .sketch import DEFAULT_SUB_BITS, decode_timeline_sketch, timeline_sketch_device, timeline_sketch_out_words
from .timeline import decode_timeline, timeline_device, timeline_out_words

MAX_PERIOD_NS = 1 << 40


def closed_loop_workspace_bytes(n: int, connections: int) -> int:
    b = C.c_uint64()
    native.check(native.load().isim_closed_loop_workspace_bytes(n, connections, C.byref(b)))
    return int(b.value)


def decode_closed_loop_info(info) -> dict:
    return {"makespan_ns": int(info[native.CL_MAKESPAN]), "min_free_ns": int(info[native.CL_MIN_FREE]),
            "late": int(info[native.CL_LATE]), "sum_late_ns": int(info[native.CL_SUM_LATE])}


class ClosedLoop:
    """C connections; qps=None is "max"; qps q gives each connection the period C * 10^9 // q ns
    (or give period_ns itself); uniform staggers the connections' slots (Fortio's -uniform)."""

    def __init__(self, connections: int = 64, qps=None, period_ns=None, uniform: bool = False):
        self.connections = int(connections)
        if qps is not None and period_ns is not None:
            raise ValueError("give qps or period_ns, not both")
        if qps is not None:
            if not qps > 0:
                raise ValueError("qps must be positive (None for max)")
            period_ns = int(self.connections * 10**9 // qps)
            if not 1 <= period_ns <= MAX_PERIOD_NS:
                raise ValueError("qps gives a period outside 1 .. 2^40 ns per connection")
        self.period_ns = int(period_ns or 0)
        self.uniform = bool(uniform)

    def __repr__(self) -> str:
        return f"ClosedLoop(connections={self.connections}, period_ns={self.period_ns}, uniform={self.uniform})"

    def c(self, first_index: int = 0) -> native.ClosedLoop:
        """The isim_closed_loop of a batch that starts at request first_index."""
        return native.ClosedLoop(self.connections, native.CL_UNIFORM if self.uniform else 0, self.period_ns,
                                 int(first_index))

    def schedule(self, j: int) -> tuple:
        """(connection, scheduled start in ns) of request j."""
        cl, c, s = self.c(), C.c_uint32(), C.c_uint64()
        native.check(native.load().isim_closed_loop_schedule(C.byref(cl), int(j), C.byref(c), C.byref(s)))
        return int(c.value), int(s.value)

    def _state(self, free_at):
        if free_at is None:
            return np.zeros(max(1, self.connections), np.uint64)
        f = np.array(free_at, dtype=np.uint64, order="C")       # a copy: the caller's state stays
        if f.shape != (self.connections,):
            raise ValueError("free_at must hold one u64 per connection")
        return f

    def _sync(self, fn, head, records, first_index, free_at):
        recs = np.ascontiguousarray(records, dtype=REC_DTYPE)
        n = len(recs)
        f, arr, info = self._state(free_at), np.zeros(n, np.uint64), np.zeros(native.CL_INFO_WORDS, np.uint64)
        cl = self.c(first_index)
        native.check(fn(*head, C.byref(cl), recs.ctypes.data if n else None, n, f.ctypes.data,
                        arr.ctypes.data if n else None, info.ctypes.data))
        return arr, f, info

    def arrivals(self, records, first_index: int = 0, free_at=None, device: int = 0):
        """Synchronous, on the GPU: (arrivals u64[n], free_at u64[C] after the batch, info u64[4])."""
        return self._sync(native.load().isim_closed_loop, (device,), records, first_index, free_at)

    def arrivals_host(self, records, first_index: int = 0, free_at=None):
        """The same on the host (the rule as a sequential loop, no GPU)."""
        return self._sync(native.load().isim_closed_loop_host, (), records, first_index, free_at)

    def arrivals_device(self, d_records: int, n: int, first_index: int = 0, *, d_free_at: int = 0, d_arrivals: int,
                        d_info: int, d_workspace: int, workspace_bytes: int = None, stream: int = 0) -> None:
        """Asynchronous on the current HIP device; pointers are device addresses.  d_free_at
        (C u64, 0: zeros in, nothing out) is read and overwritten, d_arrivals (n u64) and d_info
        (4 u64) are written; d_workspace: closed_loop_workspace_bytes(n, C) bytes, dirty or not."""
        if workspace_bytes is None:
            workspace_bytes = closed_loop_workspace_bytes(n, self.connections)
        cl = self.c(first_index)
        native.check(native.load().isim_closed_loop_device(C.byref(cl), d_records or None, n, d_free_at or None,
                                                           d_arrivals or None, d_info or None, d_workspace or None,
                                                           workspace_bytes, stream or None))


class ClosedLoopRun:
    """A closed-loop load test of a walk for duration_ns of simulated time: batches of `batch`
    traces served on the device, their arrivals from the client with free_at chained, each batch
    folded into one timeline table (n_windows = duration_ns / window_ns, which must divide) and
    one timeline sketch.  The run stops once every connection is free at or after duration_ns
    (ISIM_CL_MIN_FREE), so every request that starts inside the duration has been served;
    requests that start at or after it fall in the "after" row."""

    def __init__(self, handler, client: ClosedLoop, duration_ns: int, window_ns: int, batch: int = 1 << 16,
                 sub_bits: int = DEFAULT_SUB_BITS, max_requests: int = 1 << 30):
        if duration_ns < 1 or window_ns < 1 or batch < 1:
            raise ValueError("duration_ns, window_ns and batch must be positive")
        if duration_ns % window_ns:
            raise ValueError("window_ns must divide duration_ns: the last window ends with the run")
        self.handler, self.client = handler, client
        self.duration_ns, self.window_ns, self.batch, self.sub_bits = int(duration_ns), int(window_ns), int(batch), sub_bits
        self.n_windows = self.duration_ns // self.window_ns
        self.max_requests = int(max_requests)     # a walk of latency 0 at qps "max" never passes the duration
        if self.n_windows > native.TL_MAX_WINDOWS:
            raise ValueError("duration_ns / window_ns is above the timeline's 65536 windows")

    def run(self, trace_begin: int = 0, device: int = 0, q=None) -> dict:
        """{"timeline": decode_timeline, "sketch": decode_timeline_sketch, "timeline_table" /
        "sketch_table": the raw tables, "requests": those that start inside the duration,
        "served": all records served, "achieved_qps", "info": the last batch's totals,
        "late" / "sum_late_ns": over the run, "free_at"}."""
        import torch
        dev = torch.device("cuda", device)
        C_, nb, W = self.client.connections, self.batch, self.n_windows
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream

            def i64(words):
                return torch.zeros(max(1, words), dtype=torch.int64, device=dev)

            recs, arr, free_at, info = i64(2 * nb), i64(nb), i64(C_), i64(native.CL_INFO_WORDS)
            stats = i64(self.handler.stats_words)
            table, sketch = i64(timeline_out_words(W)), i64(timeline_sketch_out_words(W, self.sub_bits))
            wsb = closed_loop_workspace_bytes(nb, C_)
            ws = torch.empty(max(1, wsb), dtype=torch.uint8, device=dev)
            served = late = sum_late = 0
            while True:
                self.handler.serve_device(trace_begin + served, nb, recs.data_ptr(), stats.data_ptr(), stream)
                self.client.arrivals_device(recs.data_ptr(), nb, served, d_free_at=free_at.data_ptr(),
                                            d_arrivals=arr.data_ptr(), d_info=info.data_ptr(),
                                            d_workspace=ws.data_ptr(), workspace_bytes=wsb, stream=stream)
                timeline_device(arr.data_ptr(), recs.data_ptr(), nb, self.window_ns, W, d_out=table.data_ptr(),
                                stream=stream)
                timeline_sketch_device(arr.data_ptr(), recs.data_ptr(), nb, self.window_ns, W, 0, self.sub_bits,
                                       d_out=sketch.data_ptr(), stream=stream)
                served += nb
                h_info = info.cpu().numpy().view(np.uint64)       # waits for the batch
                late += int(h_info[native.CL_LATE])
                sum_late += int(h_info[native.CL_SUM_LATE])
                if int(h_info[native.CL_MIN_FREE]) >= self.duration_ns:
                    break
                if served >= self.max_requests:
                    raise RuntimeError(f"closed-loop run: {served} requests served and a connection is still free "
                                       f"at {int(h_info[native.CL_MIN_FREE])} ns, before duration_ns")
            h_table = table.cpu().numpy().view(np.uint64)
            h_sketch = sketch.cpu().numpy().view(np.uint64)
            h_free = free_at.cpu().numpy().view(np.uint64)
        tl = decode_timeline(h_table, W, 0, self.window_ns)
        kw = {} if q is None else {"q": q}
        requests = int(tl["arrived"].sum())       # no arrival is before 0: the windows hold all that start inside
        return {"timeline": tl, "sketch": decode_timeline_sketch(h_sketch, W, 0, self.window_ns, self.sub_bits, **kw),
                "timeline_table": h_table, "sketch_table": h_sketch, "requests": requests, "served": served,
                "achieved_qps": requests * 1e9 / self.duration_ns, "info": decode_closed_loop_info(h_info),
                "late": late, "sum_late_ns": sum_late & ((1 << 64) - 1), "free_at": h_free}
