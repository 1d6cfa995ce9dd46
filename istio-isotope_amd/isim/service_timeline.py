"""Service timeline: per-service queue depth and utilisation over time.

    d = isim.DesHandler(handler, profile=isim.LoadProfile.spikes(...))      # a DES on the item engine
    t = d.service_timeline(0, n, window_ns=1_000_000, n_windows=200)        # the whole batch, folded on the GPU
    print(t.to_text(top=5))                                                 # the busiest services and their peak
    t.utilisation()[s], t.mean_queue()[s], t.queue_depth()[s]               # per window of service s

The servers' side of a load test: the spans of a whole tapped batch
(isim_serve_des_spans*, threshold 0) folded into a (service x window) table
(isim_service_timeline*): per service and window the invocations that
arrived, started and finished, their queue waits, the integral of the queue
length and the worker-busy time.  Tables merge across batches, shards and GPUs.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import native
from .des_spans import DES_SPAN_DTYPE


def _params(window_ns: int, n_windows: int, t0_ns: int) -> native.TimelineParams:
    return native.TimelineParams(int(t0_ns), int(window_ns), int(n_windows), 0)


def service_holds(handler):
    """isim_des_service_holds: (hold_ns u64[n_services], replicas u32[n_services])."""
    n = int(handler.info.n_services)
    hold, reps = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    native.check(native.load().isim_des_service_holds(handler._h, hold.ctypes.data, reps.ctypes.data))
    return hold, reps


def service_workers(handler) -> np.ndarray:
    """isim_des_workers_get: workers per replica u32[n_services] (1 each until set)."""
    w = np.zeros(int(handler.info.n_services), np.uint32)
    native.check(native.load().isim_des_workers_get(handler._h, w.ctypes.data))
    return w


def service_timeline_table_words(handler, window_ns: int, n_windows: int, t0_ns: int = 0) -> int:
    b = C.c_uint64()
    native.check(native.load().isim_service_timeline_table_words(
        handler._h, C.byref(_params(window_ns, n_windows, t0_ns)), C.byref(b)))
    return int(b.value)


def service_timeline_workspace_bytes(handler, window_ns: int, n_windows: int, t0_ns: int = 0) -> int:
    b = C.c_uint64()
    native.check(native.load().isim_service_timeline_workspace_bytes(
        handler._h, C.byref(_params(window_ns, n_windows, t0_ns)), C.byref(b)))
    return int(b.value)


def service_timeline_device(handler, window_ns: int, n_windows: int, t0_ns: int, d_off: int, d_spans: int,
                            cap_spans: int, d_info: int, d_table: int, d_workspace: int, workspace_bytes: int,
                            stream: int = 0) -> None:
    """isim_service_timeline_device over device addresses: folds the spans a preceding serve_spans_device on
    the same stream wrote and adds into d_table."""
    native.check(native.load().isim_service_timeline_device(
        handler._h, C.byref(_params(window_ns, n_windows, t0_ns)), d_off or None, d_spans or None, cap_spans,
        d_info or None, d_table or None, d_workspace or None, workspace_bytes, stream or None))


def _fold(handler, spans, window_ns, n_windows, t0_ns, table, device):
    spans = np.ascontiguousarray(spans, dtype=DES_SPAN_DTYPE)
    if table is None:
        table = np.zeros(service_timeline_table_words(handler, window_ns, n_windows, t0_ns), np.uint64)
    p = _params(window_ns, n_windows, t0_ns)
    sp = spans.ctypes.data if len(spans) else None
    lib = native.load()
    if device is None:
        native.check(lib.isim_service_timeline_host(handler._h, C.byref(p), sp, len(spans), table.ctypes.data))
    else:
        native.check(lib.isim_service_timeline(device, handler._h, C.byref(p), sp, len(spans), table.ctypes.data))
    return table


def service_timeline_host(handler, spans: np.ndarray, window_ns: int, n_windows: int, t0_ns: int = 0,
                          table: np.ndarray = None) -> np.ndarray:
    """isim_service_timeline_host: the fold on the CPU over a DES_SPAN_DTYPE array; `table` (flat u64) is
    added into, a new one otherwise.  Returns the flat table."""
    return _fold(handler, spans, window_ns, n_windows, t0_ns, table, None)


def service_timeline(handler, spans: np.ndarray, window_ns: int, n_windows: int, t0_ns: int = 0, device: int = 0,
                     table: np.ndarray = None) -> np.ndarray:
    """isim_service_timeline: the same fold on GPU `device`, host arrays in and out."""
    return _fold(handler, spans, window_ns, n_windows, t0_ns, table, device)


class ServiceTimeline:
    """A service timeline table.  table: u64 [n_services][n_windows + 2][SVT_ROW_WORDS] (row
    0 before t0_ns, rows 1 .. n_windows the windows, the last row after them); header: the spans folded and
    refused.  Every word is a sum except SVT_MAX_WAIT, which merges by max."""

    def __init__(self, handler, window_ns: int, n_windows: int, t0_ns: int = 0, table: np.ndarray = None,
                 names: Sequence[str] = None):
        self.handler = handler
        self.window_ns, self.n_windows, self.t0_ns = int(window_ns), int(n_windows), int(t0_ns)
        self.names = names if names is not None else [s["name"] for s in handler.graph.canonical()["services"]]
        words = service_timeline_table_words(handler, window_ns, n_windows, t0_ns)
        self.flat = np.zeros(words, np.uint64) if table is None else np.ascontiguousarray(table, dtype=np.uint64).ravel()
        assert self.flat.size == words
        self.hold_ns, self.replicas = service_holds(handler)
        self.workers = service_workers(handler)   # as the handler has them now: those of the batches folded

    @property
    def table(self) -> np.ndarray:
        W = native.SVT_ROW_WORDS
        return self.flat[:-W].reshape(len(self.names), self.n_windows + 2, W)

    @property
    def header(self) -> dict:
        h = self.flat[-native.SVT_ROW_WORDS:]
        return dict(folded=int(h[native.SVT_H_FOLDED]), refused=int(h[native.SVT_H_REFUSED]))

    def utilisation(self) -> np.ndarray:
        """[n_services][n_windows] floats: BUSY_NS / (window_ns x replicas x workers)."""
        busy = self.table[:, 1:-1, native.SVT_BUSY_NS].astype(np.float64)
        servers = self.replicas.astype(np.float64) * self.workers.astype(np.float64)
        return busy / (float(self.window_ns) * servers[:, None])

    def mean_queue(self) -> np.ndarray:
        """[n_services][n_windows] floats: the mean queue length QUEUED_NS / window_ns."""
        return self.table[:, 1:-1, native.SVT_QUEUED_NS].astype(np.float64) / float(self.window_ns)

    def queue_depth(self) -> np.ndarray:
        """[n_services][n_windows + 2] u64: the requests queued at the end of each row, the cumulative
        ARRIVED - STARTED over the rows up to it (a start never precedes its arrival, so u64 holds it)."""
        t = self.table
        return np.cumsum(t[:, :, native.SVT_ARRIVED], axis=1, dtype=np.uint64) \
            - np.cumsum(t[:, :, native.SVT_STARTED], axis=1, dtype=np.uint64)

    def merge(self, other: "ServiceTimeline") -> "ServiceTimeline":
        """isim_service_timeline_merge: adds other's table, the maxima by max."""
        assert (self.window_ns, self.n_windows, self.t0_ns) == (other.window_ns, other.n_windows, other.t0_ns)
        native.check(native.load().isim_service_timeline_merge(
            self.handler._h, C.byref(_params(self.window_ns, self.n_windows, self.t0_ns)), self.flat.ctypes.data,
            other.flat.ctypes.data))
        return self

    def to_text(self, top: int = None) -> str:
        """The busiest services (by worker-busy time over all rows) with their peak-utilisation window."""
        h, t = self.header, self.table
        pooled = bool((self.workers > 1).any())   # the workers column only when some service has a pool
        lines = [f"service timeline of {h['folded']} spans: {self.n_windows} windows of {self.window_ns} ns from "
                 f"{self.t0_ns} ns" + (f", {h['refused']} refused" if h["refused"] else ""),
                 f"{'service':<24}{'replicas':>9}" + (f"{'workers':>8}" if pooled else "") + f"{'busy_ns':>16}{'peak util':>10}{'at window':>10}{'peak queue':>11}"
                 f"{'max_wait_ns':>14}{'invocations':>12}"]
        util, queue = self.utilisation(), self.mean_queue()
        busy = t[:, :, native.SVT_BUSY_NS].sum(axis=1, dtype=np.uint64)
        order = [s for s in np.argsort(-busy.astype(np.float64), kind="stable")
                 if int(t[s, :, native.SVT_ARRIVED].sum())]
        for s in order[:top]:
            w = int(np.argmax(util[s]))
            lines.append(f"{self.names[s]:<24}{int(self.replicas[s]):>9}"
                         + (f"{int(self.workers[s]):>8}" if pooled else "") + f"{int(busy[s]):>16}{util[s, w]:>10.3f}{w:>10}"
                         f"{queue[s].max():>11.2f}{int(t[s, :, native.SVT_MAX_WAIT].max()):>14}"
                         f"{int(t[s, :, native.SVT_ARRIVED].sum()):>12}")
        return "\n".join(lines)
