"""Trace spans: the executed invocations of chosen traces.

    ts = isim.TraceSpans(handler)                    # a dynamic walk (or ISIM_FLAG_DYNAMIC)
    recs, _ = handler.serve(0, n)
    for t in ts.slowest(recs, 0):                    # the traces at or above p99.9, at most 64
        print(t.to_text())
    t = ts.spans([12345])[0]                         # any trace, from its id alone
    cp = ts.tail_critical_path(recs, 0)              # across the tail: which services hold the latency (§20)
    print(cp.to_text())

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


def _i64(words, dev):
    import torch
    return torch.zeros(max(1, words), dtype=torch.int64, device=dev)


class Trace:
    """One trace: its id, its spans (a SPAN_DTYPE array ordered by hop) and the graph's service names."""

    def __init__(self, trace_id: int, spans: np.ndarray, names: Sequence[str]):
        self.trace_id, self.spans, self.names = int(trace_id), spans, names

    @property
    def latency_ns(self) -> int:
        return int(self.spans["duration_ns"][0])

    def __len__(self) -> int:
        return len(self.spans)

    def critical(self) -> np.ndarray:
        """The hops on the critical path (set by TraceSpans.critical_path*; empty before)."""
        return np.flatnonzero(self.spans["status"] & native.SPAN_CRITICAL)

    def to_text(self) -> str:
        """An indented tree: service, status, start and duration per executed invocation; a span on the
        critical path ends in " *"."""
        s = self.spans
        depth = np.zeros(len(s), np.int64)
        lines = [f"trace {self.trace_id}: {len(s)} spans, {self.latency_ns} ns"]
        for i in range(len(s)):
            if i:
                depth[i] = depth[s["caller_hop"][i]] + 1
            st = int(s["status"][i])
            code = "200" if not st & 1 else ("500" if st & 2 else "500 (failed step)")
            lines.append(f"{'  ' * int(depth[i])}{self.names[int(s['service'][i])]} {code} "
                         f"start={int(s['start_ns'][i])} hop={int(s['hop_ns'][i])} dur={int(s['duration_ns'][i])}"
                         f"{' *' if st & native.SPAN_CRITICAL else ''}")
        return "\n".join(lines)


CP_WORDS = ("invocations", "sum_duration_ns", "critical", "self_ns", "hop_ns", "critical_500")


class CriticalPath:
    """A critical-path table: per service the six ISIM_CP_* words, then the header row;
    every word a sum mod 2^64, so tables of calls, batches, shards and GPUs merge by addition.  traces:
    the marked Traces, where the call kept them."""

    def __init__(self, handler, table: np.ndarray, names: Sequence[str], traces: List[Trace] = None):
        self.handler, self.names, self.traces = handler, names, list(traces or [])
        self.table = np.ascontiguousarray(table, dtype=np.uint64).reshape(len(names) + 1, native.CP_ROW_WORDS)

    @property
    def header(self) -> dict:
        h = self.table[-1]
        return dict(traces=int(h[native.CP_H_TRACES]), spans=int(h[native.CP_H_SPANS]),
                    critical=int(h[native.CP_H_CRITICAL]), sum_latency_ns=int(h[native.CP_H_SUM_LATENCY]),
                    refused=int(h[native.CP_H_REFUSED]))

    def rows(self) -> List[dict]:
        """Per service with an invocation: its name, the six words and its share of the latency (SELF_NS +
        HOP_NS over the header's sum), sorted by that time, the largest first."""
        total = self.header["sum_latency_ns"]
        out = []
        for name, r in zip(self.names, self.table[:-1]):
            if not int(r[native.CP_INVOCATIONS]):
                continue
            d = dict(service=name, **{w: int(x) for w, x in zip(CP_WORDS, r)})
            d["path_ns"] = d["self_ns"] + d["hop_ns"]
            d["share"] = d["path_ns"] / total if total else 0.0
            out.append(d)
        return sorted(out, key=lambda d: -d["path_ns"])

    def merge(self, other: "CriticalPath") -> "CriticalPath":
        """Adds other's table (isim_critical_path_merge) and takes its traces along."""
        assert self.table.shape == other.table.shape
        native.check(native.load().isim_critical_path_merge(self.handler._h, self.table.ctypes.data,
                                                            other.table.ctypes.data))
        self.traces += other.traces
        return self

    def to_text(self, top: int = None) -> str:
        h = self.header
        lines = [f"critical path of {h['traces']} traces: {h['critical']} of {h['spans']} spans, "
                 f"{h['sum_latency_ns']} ns" + (f", {h['refused']} refused" if h["refused"] else ""),
                 f"{'service':<24}{'share':>8}{'self_ns':>16}{'hop_ns':>14}{'critical':>10}{'of':>10}{'500':>8}"]
        for d in self.rows()[:top]:
            lines.append(f"{d['service']:<24}{100 * d['share']:>7.2f}%{d['self_ns']:>16}{d['hop_ns']:>14}"
                         f"{d['critical']:>10}{d['invocations']:>10}{d['critical_500']:>8}")
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

    # ---- the critical path
    def table_words(self) -> int:
        w = C.c_uint64()
        native.check(native.load().isim_critical_path_table_words(self.handler._h, C.byref(w)))
        return int(w.value)

    def critical_path_workspace_bytes(self, cap_spans: int) -> int:
        b = C.c_uint64()
        native.check(native.load().isim_critical_path_workspace_bytes(self.handler._h, cap_spans, C.byref(b)))
        return int(b.value)

    def fold_host(self, off: np.ndarray, spans: np.ndarray, n_written: int, table: np.ndarray = None) -> np.ndarray:
        """isim_critical_path_host over host spans, in place (start_ns, the critical bit); adds into table
        (a new one of zeros when None) and returns it."""
        if table is None:
            table = np.zeros(self.table_words(), np.uint64)
        native.check(native.load().isim_critical_path_host(self.handler._h, off.ctypes.data, n_written,
                                                           spans.ctypes.data, table.ctypes.data))
        return table

    def fold(self, off: np.ndarray, spans: np.ndarray, n_written: int, table: np.ndarray = None,
             device: int = 0) -> np.ndarray:
        """The same through isim_critical_path: on the GPU, synchronous, over host buffers."""
        if table is None:
            table = np.zeros(self.table_words(), np.uint64)
        native.check(native.load().isim_critical_path(device, self.handler._h, off.ctypes.data, n_written,
                                                      spans.ctypes.data, table.ctypes.data))
        return table

    def critical_path(self, ids, device: int = 0) -> CriticalPath:
        """Synchronous, on the GPU: the spans of the listed traces and their critical path."""
        ids, off, spans, info = self._raw(native.load().isim_trace_spans, (device,), ids, None)
        written = int(info[native.SPAN_WRITTEN])
        table = self.fold(off, spans, written, device=device)
        return CriticalPath(self.handler, table, self.names, self._split(ids, off, spans, written))

    def critical_path_host(self, ids) -> CriticalPath:
        """The same on the host (no GPU)."""
        ids, off, spans, info = self._raw(native.load().isim_trace_spans_host, (), ids, None)
        written = int(info[native.SPAN_WRITTEN])
        table = self.fold_host(off, spans, written)
        return CriticalPath(self.handler, table, self.names, self._split(ids, off, spans, written))

    def critical_path_device(self, *, d_off: int, d_spans: int, cap_spans: int, d_info: int, n_ids: int, d_table: int,
                             d_workspace: int, workspace_bytes: int = None, stream: int = 0) -> None:
        """Asynchronous on the current HIP device, after a spans_device call of n_ids entries with the
        same d_off, d_spans, cap_spans and d_info: fills start_ns, marks the critical spans and ADDS into
        d_table (table_words() u64, zeroed by the caller); d_workspace:
        critical_path_workspace_bytes(cap_spans) bytes, dirty or not."""
        if workspace_bytes is None:
            workspace_bytes = self.critical_path_workspace_bytes(cap_spans)
        native.check(native.load().isim_critical_path_device(self.handler._h, d_off or None, d_spans or None,
                                                             cap_spans, d_info or None, n_ids, d_table or None,
                                                             d_workspace or None, workspace_bytes, stream or None))

    def _tail_ids(self, records, trace_begin, q_ppm, cls, max_traces, dev, stream):
        """(ids as a device tensor, how many) of the records at or above their exact q_ppm latency quantile
        in class cls, the first max_traces (None: all) in trace order: the quantile select and the trace
        select on `stream`.  Call with `dev` current."""
        import torch
        if isinstance(records, torch.Tensor):
            d_recs, n = records, records.numel() * records.element_size() // REC_DTYPE.itemsize
        else:
            recs = np.ascontiguousarray(records, dtype=REC_DTYPE)
            n = len(recs)
            d_recs = torch.from_numpy(recs.view(np.int64).copy()).to(dev)
        if n == 0:
            return None, 0
        keep = n if max_traces is None else min(int(max_traces), n)
        q = (q_ppm / 1e6,)
        qout = _i64(quantiles_out_words(1), dev)
        qws = torch.empty(quantiles_workspace_bytes(1), dtype=torch.uint8, device=dev)
        latency_quantiles_device(d_recs.data_ptr(), n, q, d_out=qout.data_ptr(), d_workspace=qws.data_ptr(),
                                 stream=stream)
        # the select takes its threshold by value: the one word the host reads between the steps
        thr = int(qout.cpu().numpy().view(np.uint64).reshape(3, 2)[cls, 1])
        ids, sinfo = _i64(keep, dev), _i64(2, dev)
        sws = torch.empty(select_workspace_bytes(n), dtype=torch.uint8, device=dev)
        select_traces_device(d_recs.data_ptr(), n, trace_begin, thr, cls, max_ids=keep,
                             d_ids=ids.data_ptr(), d_info=sinfo.data_ptr(), d_workspace=sws.data_ptr(),
                             stream=stream)
        return ids, int(sinfo.cpu().numpy().view(np.uint64)[1])

    def slowest(self, records, trace_begin: int, q_ppm: int = 999000, cls: int = native.Q_ALL, max_traces: int = 64,
                device: int = 0) -> List[Trace]:
        """The traces of a served batch at or above its exact q_ppm latency quantile in class cls (the
        first max_traces in trace order): the quantile select, the trace select and the span walks on
        one stream of the device.  records: a host REC_DTYPE array, or a torch tensor on the device."""
        import torch
        dev = torch.device("cuda", device)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            ids, m = self._tail_ids(records, trace_begin, q_ppm, cls, max_traces, dev, stream)
            if m == 0:
                return []
            off, info = _i64(m + 1, dev), _i64(native.SPAN_INFO_WORDS, dev)
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

    def tail_critical_path(self, records, trace_begin: int, q_ppm: int = 999000, cls: int = native.Q_ALL,
                           max_traces: int = None, cap_spans: int = 1 << 20, keep_traces: bool = False,
                           device: int = 0) -> CriticalPath:
        """The critical path across the tail of a served batch: the traces at or above its exact q_ppm
        latency quantile in class cls (all of them, or the first max_traces in trace order).  Four steps
        on one stream of the device: quantile, select, spans, critical path; the last two in chunks of
        what a buffer of cap_spans spans holds (the next chunk starts at ISIM_SPAN_FIRST_UNFIT), all
        adding into one table.  keep_traces: the marked Traces come along (copied to the host)."""
        import torch
        dev = torch.device("cuda", device)
        words = self.table_words()
        traces: List[Trace] = []
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            ids, m = self._tail_ids(records, trace_begin, q_ppm, cls, max_traces, dev, stream)
            table = _i64(words, dev)
            cap, pos = max(1, int(cap_spans)), 0
            bufs = None
            while pos < m:
                if bufs is None:    # (again after a trace that alone needs more than cap spans)
                    per = min(m, cap)       # every trace has a span: a chunk holds at most cap traces
                    off, info = _i64(per + 1, dev), _i64(native.SPAN_INFO_WORDS, dev)
                    spans = torch.empty(cap * SPAN_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                    sws_b, cws_b = self.workspace_bytes(per), self.critical_path_workspace_bytes(cap)
                    sws = torch.empty(max(1, sws_b), dtype=torch.uint8, device=dev)
                    cws = torch.empty(cws_b, dtype=torch.uint8, device=dev)
                    bufs = True
                n_ids = min(m - pos, per)
                self.spans_device(ids.data_ptr() + 8 * pos, n_ids, d_off=off.data_ptr(), d_spans=spans.data_ptr(),
                                  cap_spans=cap, d_info=info.data_ptr(), d_workspace=sws.data_ptr(),
                                  workspace_bytes=sws_b, stream=stream)
                self.critical_path_device(d_off=off.data_ptr(), d_spans=spans.data_ptr(), cap_spans=cap,
                                          d_info=info.data_ptr(), n_ids=n_ids, d_table=table.data_ptr(),
                                          d_workspace=cws.data_ptr(), workspace_bytes=cws_b, stream=stream)
                # the host reads where the next chunk starts: one word per chunk
                first_unfit = int(info.cpu().numpy().view(np.uint64)[native.SPAN_FIRST_UNFIT])
                if first_unfit == 0:    # not one trace fits: room for the first, and the chunk again
                    cap = int(off[1].item())
                    bufs = None
                    continue
                if keep_traces:
                    h_off = off[:first_unfit + 1].cpu().numpy().view(np.uint64).copy()
                    h_spans = spans[:int(h_off[-1]) * SPAN_DTYPE.itemsize].cpu().numpy().view(SPAN_DTYPE).copy()
                    h_ids = ids[pos:pos + first_unfit].cpu().numpy().view(np.uint64).copy()
                    traces += self._split(h_ids, h_off, h_spans, first_unfit)
                pos += first_unfit
            h_table = table.cpu().numpy().view(np.uint64).copy()
        return CriticalPath(self.handler, h_table, self.names, traces)
