"""DES trace spans: where the slow traces of a contended batch waited.

    d = isim.DesHandler(handler, mean_interarrival_ns=300_000)     # a DES on the item engine
    recs, stats, table, traces, waits = d.serve_spans(0, n)        # the traces at or above p99.9, at most 64
    print(traces[0].to_text())                                      # arrival, queue wait, finish per invocation
    print(waits.to_text())                                          # which service's queue held them

Under the DES an invocation's queue wait depends on every other trace of the
batch, so a trace cannot be walked again later: the tap (isim_serve_des_spans*)
writes the chosen traces' invocations out of the engine's per-batch arrays
before the batch ends, and folds their waits into a per-service table that
merges across batches and GPUs.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

import numpy as np

from . import native

DES_SPAN_DTYPE = np.dtype([("arrival_ns", "<u8"), ("start_ns", "<u8"), ("finish_ns", "<u8"), ("hop_ns", "<u8"),
                           ("hop", "<u4"), ("caller_hop", "<u4"), ("position", "<u4"), ("slot", "<u4"),
                           ("service", "<u4"), ("status", "<u4"), ("replica", "<u4"), ("reserved", "<u4")])
assert DES_SPAN_DTYPE.itemsize == 64 == C.sizeof(native.DesSpan)


def wait_table_words(handler) -> int:
    b = C.c_uint64()
    native.check(native.load().isim_des_wait_table_words(handler._h, C.byref(b)))
    return int(b.value)


class DesTrace:
    """One trace of a DES batch: its id, its spans (a DES_SPAN_DTYPE array ordered by hop, times on the
    batch clock) and the graph's service names."""

    def __init__(self, trace_id: int, spans: np.ndarray, names: Sequence[str]):
        self.trace_id, self.spans, self.names = int(trace_id), spans, names

    @property
    def arrival_ns(self) -> int:
        return int(self.spans["arrival_ns"][0])

    @property
    def latency_ns(self) -> int:
        return int(self.spans["finish_ns"][0] - self.spans["arrival_ns"][0])

    @property
    def wait_ns(self) -> np.ndarray:
        """The queue wait S - a of every span."""
        return self.spans["start_ns"] - self.spans["arrival_ns"]

    def __len__(self) -> int:
        return len(self.spans)

    def to_text(self) -> str:
        """An indented tree: service, replica, status, arrival relative to the trace's, queue wait and
        duration (finish - arrival) per executed invocation; a span on the critical path (DesCriticalPath)
        ends in " *"."""
        s = self.spans
        a0 = self.arrival_ns
        depth = np.zeros(len(s), np.int64)
        lines = [f"trace {self.trace_id}: {len(s)} spans, arrived {a0} ns, {self.latency_ns} ns, "
                 f"{int(self.wait_ns.sum())} ns in queues"]
        for i in range(len(s)):
            if i:
                depth[i] = depth[s["caller_hop"][i]] + 1
            st = int(s["status"][i])
            code = "200" if not st & 1 else ("500" if st & 2 else "500 (failed step)")
            a, S, F = int(s["arrival_ns"][i]), int(s["start_ns"][i]), int(s["finish_ns"][i])
            lines.append(f"{'  ' * int(depth[i])}{self.names[int(s['service'][i])]}[{int(s['replica'][i])}] {code} "
                         f"at=+{a - a0} wait={S - a} dur={F - a}" + (" *" if st & native.SPAN_CRITICAL else ""))
        return "\n".join(lines)


DW_WORDS = ("invocations", "waited", "sum_wait_ns", "max_wait_ns", "sum_duration_ns", "resp_500")


class DesWaitTable:
    """A wait table: per service the six ISIM_DW_* words over the emitted spans, then the
    header row.  Tables of batches, shards and GPUs merge: sums by addition, MAX_WAIT by max."""

    def __init__(self, handler, table: np.ndarray = None, names: Sequence[str] = None):
        self.handler = handler
        self.names = names if names is not None else [s["name"] for s in handler.graph.canonical()["services"]]
        words = wait_table_words(handler)
        t = np.zeros(words, np.uint64) if table is None else np.ascontiguousarray(table, dtype=np.uint64)
        self.table = t.reshape(words // native.DW_ROW_WORDS, native.DW_ROW_WORDS)

    @property
    def header(self) -> dict:
        h = self.table[-1]
        return dict(traces=int(h[native.DW_H_TRACES]), spans=int(h[native.DW_H_SPANS]),
                    sum_latency_ns=int(h[native.DW_H_SUM_LATENCY]), sum_entry_wait_ns=int(h[native.DW_H_SUM_WAIT]))

    def rows(self) -> List[dict]:
        """Per service with an emitted span: its name and the six words, sorted by SUM_WAIT, the largest first."""
        out = [dict(service=name, **{w: int(x) for w, x in zip(DW_WORDS, r)})
               for name, r in zip(self.names, self.table[:-1]) if int(r[native.DW_INVOCATIONS])]
        return sorted(out, key=lambda d: -d["sum_wait_ns"])

    def merge(self, other: "DesWaitTable") -> "DesWaitTable":
        assert self.table.shape == other.table.shape
        native.check(native.load().isim_des_wait_merge(self.handler._h, self.table.ctypes.data,
                                                       other.table.ctypes.data))
        return self

    def to_text(self, top: int = None) -> str:
        h = self.header
        lines = [f"queue waits of {h['traces']} traces: {h['spans']} spans, {h['sum_latency_ns']} ns of latency",
                 f"{'service':<24}{'sum_wait_ns':>16}{'max_wait_ns':>14}{'waited':>10}{'of':>10}"
                 f"{'sum_dur_ns':>16}{'500':>8}"]
        for d in self.rows()[:top]:
            lines.append(f"{d['service']:<24}{d['sum_wait_ns']:>16}{d['max_wait_ns']:>14}{d['waited']:>10}"
                         f"{d['invocations']:>10}{d['sum_duration_ns']:>16}{d['resp_500']:>8}")
        return "\n".join(lines)


DCP_WORDS = ("invocations", "sum_duration_ns", "critical", "wait_ns", "self_ns", "hop_ns", "critical_500",
             "critical_waited")


def critical_path_table_words(handler) -> int:
    b = C.c_uint64()
    native.check(native.load().isim_des_critical_path_table_words(handler._h, C.byref(b)))
    return int(b.value)


def critical_path_workspace_bytes(handler, cap_spans: int) -> int:
    b = C.c_uint64()
    native.check(native.load().isim_des_critical_path_workspace_bytes(handler._h, cap_spans, C.byref(b)))
    return int(b.value)


def des_critical_path_device(handler, d_off: int, d_spans: int, cap_spans: int, d_info: int, n_ids: int,
                             d_table: int, d_trace_wait: int, d_workspace: int, workspace_bytes: int,
                             stream: int = 0) -> None:
    """isim_des_critical_path_device over device addresses: folds the traces a preceding
    serve_spans_device on the same stream wrote, adds into d_table, marks the spans in place."""
    native.check(native.load().isim_des_critical_path_device(
        handler._h, d_off, d_spans or None, cap_spans, d_info, n_ids, d_table, d_trace_wait or None,
        d_workspace or None, workspace_bytes, stream or None))


def des_critical_path_host(handler, off: np.ndarray, n_written: int, spans: np.ndarray, table: np.ndarray,
                           trace_wait: np.ndarray = None) -> None:
    """isim_des_critical_path_host: the same fold on the CPU, in place over numpy buffers (spans a
    DES_SPAN_DTYPE array, table and trace_wait u64)."""
    native.check(native.load().isim_des_critical_path_host(
        handler._h, off.ctypes.data, n_written, spans.ctypes.data if len(spans) else None, table.ctypes.data,
        trace_wait.ctypes.data if trace_wait is not None and len(trace_wait) else None))


class DesCriticalPath:
    """A DES critical-path table: per service the eight ISIM_DCP_* words, then the header
    row; every word a sum mod 2^64, so tables of calls, batches, shards and GPUs merge by addition.
    trace_wait_ns: per folded trace the queue wait on its critical path (UINT64_MAX: refused), where the
    call kept it."""

    def __init__(self, handler, table: np.ndarray = None, names: Sequence[str] = None, trace_wait_ns=None):
        self.handler = handler
        self.names = names if names is not None else [s["name"] for s in handler.graph.canonical()["services"]]
        words = critical_path_table_words(handler)
        t = np.zeros(words, np.uint64) if table is None else np.ascontiguousarray(table, dtype=np.uint64)
        self.table = t.reshape(words // native.DCP_ROW_WORDS, native.DCP_ROW_WORDS)
        self.trace_wait_ns = np.zeros(0, np.uint64) if trace_wait_ns is None else np.asarray(trace_wait_ns, np.uint64)

    @property
    def header(self) -> dict:
        h = self.table[-1]
        return dict(traces=int(h[native.DCP_H_TRACES]), spans=int(h[native.DCP_H_SPANS]),
                    critical=int(h[native.DCP_H_CRITICAL]), sum_latency_ns=int(h[native.DCP_H_SUM_LATENCY]),
                    refused=int(h[native.DCP_H_REFUSED]))

    def rows(self) -> List[dict]:
        """Per service with an invocation: its name, the eight words and its share of the latency (WAIT_NS +
        SELF_NS + HOP_NS over the header's sum), sorted by that time, the largest first."""
        total = self.header["sum_latency_ns"]
        out = []
        for name, r in zip(self.names, self.table[:-1]):
            if not int(r[native.DCP_INVOCATIONS]):
                continue
            d = dict(service=name, **{w: int(x) for w, x in zip(DCP_WORDS, r)})
            d["path_ns"] = d["wait_ns"] + d["self_ns"] + d["hop_ns"]
            d["share"] = d["path_ns"] / total if total else 0.0
            out.append(d)
        return sorted(out, key=lambda d: -d["path_ns"])

    def merge(self, other: "DesCriticalPath") -> "DesCriticalPath":
        """Adds other's table (isim_des_critical_path_merge) and takes its per-trace waits along."""
        assert self.table.shape == other.table.shape
        native.check(native.load().isim_des_critical_path_merge(self.handler._h, self.table.ctypes.data,
                                                                other.table.ctypes.data))
        self.trace_wait_ns = np.concatenate([self.trace_wait_ns, other.trace_wait_ns])
        return self

    def to_text(self, top: int = None) -> str:
        h = self.header
        lines = [f"critical path of {h['traces']} traces under load: {h['critical']} of {h['spans']} spans, "
                 f"{h['sum_latency_ns']} ns" + (f", {h['refused']} refused" if h["refused"] else ""),
                 f"{'service':<24}{'share':>8}{'wait_ns':>16}{'self_ns':>16}{'hop_ns':>14}{'critical':>10}"
                 f"{'waited':>8}{'of':>10}{'500':>8}"]
        for d in self.rows()[:top]:
            lines.append(f"{d['service']:<24}{100 * d['share']:>7.2f}%{d['wait_ns']:>16}{d['self_ns']:>16}"
                         f"{d['hop_ns']:>14}{d['critical']:>10}{d['critical_waited']:>8}{d['invocations']:>10}"
                         f"{d['critical_500']:>8}")
        return "\n".join(lines)


def make_tap(min_latency_ns: int, q_ppm: int, cls: int, max_traces: int, cap_spans: int, ids: int, off: int,
             spans: int, info: int, wait_table: int = 0) -> native.DesTap:
    """An isim_des_tap over the given addresses (device addresses for the _device call, host for the
    synchronous one)."""
    return native.DesTap(int(min_latency_ns), int(q_ppm), int(cls), int(max_traces), int(cap_spans), ids or None,
                         off or None, spans or None, info or None, wait_table or None, (C.c_uint64 * 2)(0, 0))
