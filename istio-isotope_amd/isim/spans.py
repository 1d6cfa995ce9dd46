"""Trace spans: the executed invocations of chosen traces.

    ts = isim.TraceSpans(handler)                    # a dynamic walk (or ISIM_FLAG_DYNAMIC)
    recs, _ = handler.serve(0, n)
    for t in ts.slowest(recs, 0):                    # the traces at or above p99.9, at most 64
        print(t.to_text())
    t = ts.spans([12345])[0]                         # any trace, from its id alone

A dynamic walk keeps 16 bytes per trace; a trace is a pure function of (seed,
trace id), so the calls behind any record come from walking that id again, in
libisim (isim_trace_spans_host on the host, isim_trace_spans* on the GPU).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

import numpy as np

from . import native
from .quantiles import latency_quantiles_device, quantiles_out_words, quantiles_workspace_bytes
from .sim import REC_DTYPE

SPAN_DTYPE = np.dtype([("start_ns", "<u8"), ("duration_ns", "<u8"), ("hop_ns", "<u8"), ("hop", "<u4"),
                       ("caller_hop", "<u4"), ("position", "<u4"), ("slot", "<u4"), ("service", "<u4"),
                       ("status", "<u4")])
assert SPAN_DTYPE.itemsize == 48


def select_workspace_bytes(n: int) -> int:
    b = C.c_uint64()
    native.check(native.load().isim_select_traces_workspace_bytes(n, C.byref(b)))
    return int(b.value)


def select_traces_device(d_records: int, n: int, trace_begin: int, min_latency_ns: int, cls: int = native.Q_ALL, *,
                         max_ids: int, d_ids: int, d_info: int, d_workspace: int, workspace_bytes: int = None,
                         stream: int = 0) -> None:
    """Asynchronous on the current HIP device; pointers are device addresses.  d_ids (max_ids u64)
    gets the ids trace_begin + i of the matching records in ascending i, d_info (2 u64) the matches
    and the ids written; d_workspace: select_workspace_bytes(n) bytes, dirty or not."""
    if workspace_bytes is None:
        workspace_bytes = select_workspace_bytes(n)
    native.check(native.load().isim_select_traces_device(d_records or None, n, trace_begin, min_latency_ns, cls,
                                                         max_ids, d_ids or None, d_info or None, d_workspace or None,
                                                         workspace_bytes, stream or None))


def _select(fn, head, records, trace_begin, min_latency_ns, cls, max_ids):
    recs = np.ascontiguousarray(records, dtype=REC_DTYPE)
    n = len(recs)
    keep = n if max_ids is None else int(max_ids)
    ids, info = np.zeros(max(1, min(keep, n)), np.uint64), np.zeros(2, np.uint64)
    native.check(fn(*head, recs.ctypes.data if n else None, n, trace_begin, min_latency_ns, cls, keep,
                    ids.ctypes.data, info.ctypes.data))
    return ids[:int(info[1])], int(info[0])


def select_traces(records, trace_begin: int, min_latency_ns: int, cls: int = native.Q_ALL, max_ids: int = None,
                  device: int = 0):
    """Synchronous, on the GPU: (ids u64 of the first max_ids matching records, the number of matches)."""
    return _select(native.load().isim_select_traces, (device,), records, trace_begin, min_latency_ns, cls, max_ids)


def select_traces_host(records, trace_begin: int, min_latency_ns: int, cls: int = native.Q_ALL, max_ids: int = None):
    """The same as a loop on the host (no GPU)."""
    return _select(native.load().isim_select_traces_host, (), records, trace_begin, min_latency_ns, cls, max_ids)


class Trace:
    """One trace: its id, its spans (a SPAN_DTYPE array ordered by hop) and the graph's service names."""

    def __init__(self, trace_id: int, spans: np.ndarray, names: Sequence[str]):
        self.trace_id, self.spans, self.names = int(trace_id), spans, names

    @property
    def latency_ns(self) -> int:
        return int(self.spans["duration_ns"][0])

    def __len__(self) -> int:
        return len(self.spans)

    def to_text(self) -> str:
        """An indented tree: service, status, start and duration per executed invocation."""
        s = self.spans
        depth = np.zeros(len(s), np.int64)
        lines = [f"trace {self.trace_id}: {len(s)} spans, {self.latency_ns} ns"]
        for i in range(len(s)):
            if i:
                depth[i] = depth[s["caller_hop"][i]] + 1
            st = int(s["status"][i])
            code = "200" if not st & 1 else ("500" if st & 2 else "500 (failed step)")
            lines.append(f"{'  ' * int(depth[i])}{self.names[int(s['service'][i])]} {code} "
                         f"start={int(s['start_ns'][i])} hop={int(s['hop_ns'][i])} dur={int(s['duration_ns'][i])}")
        return "\n".join(lines)


class TraceSpans:
    """The spans of a handler's traces.  ISIM_EINVAL (IsimError) for a handler without an unrolled
    tree: a static walk (create the handler with FLAG_DYNAMIC) or a walk over the site graph."""

    def __init__(self, handler):
        self.handler = handler
        self.workspace_bytes(0)  # refuses the handler here, not at the first call
        self.names = [s["name"] for s in handler.graph.canonical()["services"]]

    def workspace_bytes(self, n_ids: int) -> int:
        b = C.c_uint64()
        native.check(native.load().isim_trace_spans_workspace_bytes(self.handler._h, n_ids, C.byref(b)))
        return int(b.value)

    def _split(self, ids, off, spans, written) -> List[Trace]:
        return [Trace(ids[i], spans[int(off[i]):int(off[i + 1])], self.names) for i in range(written)]

    def _raw(self, fn, head, ids, cap_spans):
        """(offsets u64[n + 1], spans SPAN_DTYPE[cap], info u64[4]) of a synchronous entry point; cap_spans
        None: as many as the traces need (a first call with no room tells)."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        n = len(ids)
        off, info = np.zeros(n + 1, np.uint64), np.zeros(native.SPAN_INFO_WORDS, np.uint64)

        def call(cap):
            spans = np.zeros(max(1, cap), SPAN_DTYPE)
            native.check(fn(*head, self.handler._h, ids.ctypes.data if n else None, n, off.ctypes.data,
                            spans.ctypes.data, cap, info.ctypes.data))
            return spans[:cap]

        if cap_spans is None:
            call(0)
            cap_spans = int(info[native.SPAN_TOTAL])
        return ids, off, call(int(cap_spans)), info

    def raw(self, ids, cap_spans: int = None, device: int = 0):
        ids, off, spans, info = self._raw(native.load().isim_trace_spans, (device,), ids, cap_spans)
        return off, spans, info

    def raw_host(self, ids, cap_spans: int = None):
        ids, off, spans, info = self._raw(native.load().isim_trace_spans_host, (), ids, cap_spans)
        return off, spans, info

    def spans(self, ids, device: int = 0) -> List[Trace]:
        """Synchronous, on the GPU: one Trace per listed id (any u64, unsorted, repeats allowed)."""
        ids, off, spans, info = self._raw(native.load().isim_trace_spans, (device,), ids, None)
        return self._split(ids, off, spans, int(info[native.SPAN_WRITTEN]))

    def spans_host(self, ids) -> List[Trace]:
        """The same walk on the host (no GPU)."""
        ids, off, spans, info = self._raw(native.load().isim_trace_spans_host, (), ids, None)
        return self._split(ids, off, spans, int(info[native.SPAN_WRITTEN]))

    def spans_device(self, d_trace_ids: int, n_ids: int, *, d_off: int, d_spans: int, cap_spans: int, d_info: int,
                     d_workspace: int, workspace_bytes: int = None, stream: int = 0) -> None:
        """Asynchronous on the current HIP device; pointers are device addresses.  d_off (n_ids + 1
        u64), d_spans (cap_spans spans) and d_info (4 u64) are written; start_ns stays 0 (place()
        fills it on the host); d_workspace: workspace_bytes(n_ids) bytes, dirty or not."""
        if workspace_bytes is None:
            workspace_bytes = self.workspace_bytes(n_ids)
        native.check(native.load().isim_trace_spans_device(self.handler._h, d_trace_ids or None, n_ids, d_off or None,
                                                           d_spans or None, cap_spans, d_info or None,
                                                           d_workspace or None, workspace_bytes, stream or None))

    def place(self, off: np.ndarray, spans: np.ndarray, n_written: int) -> None:
        """Fills start_ns of the first n_written traces of a spans_device result copied to the host."""
        native.check(native.load().isim_trace_spans_place(self.handler._h, off.ctypes.data, n_written,
                                                          spans.ctypes.data))

    def slowest(self, records, trace_begin: int, q_ppm: int = 999000, cls: int = native.Q_ALL, max_traces: int = 64,
                device: int = 0) -> List[Trace]:
        """The traces of a served batch at or above its exact q_ppm latency quantile in class cls (the
        first max_traces in trace order): the quantile select, the trace select and the span walks on
        one stream of the device.  records: a host REC_DTYPE array, or a torch tensor on the device."""
        import torch
        dev = torch.device("cuda", device)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            if isinstance(records, torch.Tensor):
                d_recs, n = records, records.numel() * records.element_size() // REC_DTYPE.itemsize
            else:
                recs = np.ascontiguousarray(records, dtype=REC_DTYPE)
                n = len(recs)
                d_recs = torch.from_numpy(recs.view(np.int64).copy()).to(dev)
            if n == 0:
                return []

            def i64(words):
                return torch.zeros(max(1, words), dtype=torch.int64, device=dev)

            q = (q_ppm / 1e6,)
            qout = i64(quantiles_out_words(1))
            qws = torch.empty(quantiles_workspace_bytes(1), dtype=torch.uint8, device=dev)
            latency_quantiles_device(d_recs.data_ptr(), n, q, d_out=qout.data_ptr(), d_workspace=qws.data_ptr(),
                                     stream=stream)
            # the select takes its threshold by value: the one word the host reads between the steps
            thr = int(qout.cpu().numpy().view(np.uint64).reshape(3, 2)[cls, 1])
            ids, sinfo = i64(max_traces), i64(2)
            sws = torch.empty(select_workspace_bytes(n), dtype=torch.uint8, device=dev)
            select_traces_device(d_recs.data_ptr(), n, trace_begin, thr, cls, max_ids=max_traces,
                                 d_ids=ids.data_ptr(), d_info=sinfo.data_ptr(), d_workspace=sws.data_ptr(),
                                 stream=stream)
            m = int(sinfo.cpu().numpy().view(np.uint64)[1])
            if m == 0:
                return []
            off, info = i64(m + 1), i64(native.SPAN_INFO_WORDS)
            wsb = self.workspace_bytes(m)
            ws = torch.empty(max(1, wsb), dtype=torch.uint8, device=dev)
            cap = min(m * max(1, int(self.handler.info.hops_upper)), 1 << 20)
            while True:
                spans = torch.empty(max(1, cap) * SPAN_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                self.spans_device(ids.data_ptr(), m, d_off=off.data_ptr(), d_spans=spans.data_ptr(), cap_spans=cap,
                                  d_info=info.data_ptr(), d_workspace=ws.data_ptr(), workspace_bytes=wsb,
                                  stream=stream)
                h_info = info.cpu().numpy().view(np.uint64)
                if int(h_info[native.SPAN_WRITTEN]) == m:
                    break
                cap = int(h_info[native.SPAN_TOTAL])
            h_off = off.cpu().numpy().view(np.uint64).copy()
            total = int(h_info[native.SPAN_TOTAL])
            h_spans = spans[:total * SPAN_DTYPE.itemsize].cpu().numpy().view(SPAN_DTYPE).copy()
            h_ids = ids.cpu().numpy().view(np.uint64)[:m].copy()
        self.place(h_off, h_spans, m)
        return self._split(h_ids, h_off, h_spans, m)
