"""Per-service exact percentiles over time: p99 by service and window.

    d = isim.DesHandler(handler, profile=isim.LoadProfile.spikes(...))       # a DES on the item engine
    wq = d.service_window_quantiles(0, n, q=(0.5, 0.99), window_ns=1_000_000, n_windows=200)
    wq.series("cart", "duration", 0.99)                    # u64[n_windows + 2]: the p99 duration of cart per row
    wq.worst("wait", 0.99, 3)                              # [(name, row, ns)] of the three largest p99 queue waits
    print(wq.to_text(top=5))

histogram_quantile(0.99, service_request_duration_seconds) by service, over
time: the spans of a whole tapped batch (isim_serve_des_spans*, threshold 0)
grouped by service and by the timeline row (isim_timeline's rows) in which
they finish, and per cell and class (all / 200 / 500) the nearest-rank order
statistics of S - a (wait), F - S (service) and F - a (duration).  The table
is written, not added into: order statistics do not merge across batches.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import native
from .des_spans import DES_SPAN_DTYPE
from .quantiles import CLASS_NAMES, _ppm_array, q_to_ppm
from .service_quantiles import MEASURE_NAMES, _descending
from .service_timeline import _params

WAVE = native.SWQ_WAVE      # the device ranks a cell with at most this many spans in one wave's registers


def service_window_quantiles_table_words(handler, n_q: int, window_ns: int, n_windows: int, t0_ns: int = 0) -> int:
    b = C.c_uint64()
    native.check(native.load().isim_service_window_quantiles_table_words(
        handler._h, C.byref(_params(window_ns, n_windows, t0_ns)), n_q, C.byref(b)))
    return int(b.value)


def service_window_quantiles_workspace_bytes(handler, cap_spans: int, n_q: int, window_ns: int, n_windows: int,
                                             t0_ns: int = 0) -> int:
    b = C.c_uint64()
    native.check(native.load().isim_service_window_quantiles_workspace_bytes(
        handler._h, C.byref(_params(window_ns, n_windows, t0_ns)), cap_spans, n_q, C.byref(b)))
    return int(b.value)


def service_window_quantiles_device(handler, q: Sequence[float], window_ns: int, n_windows: int, t0_ns: int,
                                    d_off: int, d_spans: int, cap_spans: int, d_info: int, d_out: int,
                                    d_workspace: int, workspace_bytes: int, stream: int = 0) -> None:
    """isim_service_window_quantiles_device over device addresses: selects over the spans a preceding
    serve_spans_device on the same stream wrote and writes d_out."""
    ppm = q_to_ppm(q)
    native.check(native.load().isim_service_window_quantiles_device(
        handler._h, C.byref(_params(window_ns, n_windows, t0_ns)), _ppm_array(ppm), len(ppm), d_off or None,
        d_spans or None, cap_spans, d_info or None, d_out or None, d_workspace or None, workspace_bytes,
        stream or None))


def _table(handler, spans, q, window_ns, n_windows, t0_ns, device):
    spans = np.ascontiguousarray(spans, dtype=DES_SPAN_DTYPE)
    ppm = q_to_ppm(q)
    out = np.zeros(service_window_quantiles_table_words(handler, len(ppm), window_ns, n_windows, t0_ns), np.uint64)
    p = _params(window_ns, n_windows, t0_ns)
    sp = spans.ctypes.data if len(spans) else None
    lib = native.load()
    if device is None:
        native.check(lib.isim_service_window_quantiles_host(handler._h, C.byref(p), _ppm_array(ppm), len(ppm), sp,
                                                            len(spans), out.ctypes.data))
    else:
        native.check(lib.isim_service_window_quantiles(device, handler._h, C.byref(p), _ppm_array(ppm), len(ppm), sp,
                                                       len(spans), out.ctypes.data))
    return out


def service_window_quantiles_host(handler, spans: np.ndarray, q: Sequence[float], window_ns: int, n_windows: int,
                                  t0_ns: int = 0) -> np.ndarray:
    """isim_service_window_quantiles_host: the table on the CPU over a DES_SPAN_DTYPE array; the flat u64 table."""
    return _table(handler, spans, q, window_ns, n_windows, t0_ns, None)


def service_window_quantiles(handler, spans: np.ndarray, q: Sequence[float], window_ns: int, n_windows: int,
                             t0_ns: int = 0, device: int = 0) -> np.ndarray:
    """isim_service_window_quantiles: the same table on GPU `device`, host arrays in and out."""
    return _table(handler, spans, q, window_ns, n_windows, t0_ns, device)


def decode_service_window_quantiles(flat: np.ndarray, n_services: int, n_windows: int, n_q: int):
    """The flat table as (cells u64[n_services][n_windows + 2][3 measures][3 classes][1 + n_q],
    {"folded", "refused"})."""
    flat = np.asarray(flat, dtype=np.uint64).ravel()
    H = native.SVQ_HEADER_WORDS
    rows = n_windows + 2
    assert flat.size == n_services * rows * native.SVQ_MEASURES * native.SVQ_CLASSES * (1 + n_q) + H
    cells = flat[:-H].reshape(n_services, rows, native.SVQ_MEASURES, native.SVQ_CLASSES, 1 + n_q)
    hdr = flat[-H:]
    return cells, dict(folded=int(hdr[native.SVQ_H_FOLDED]), refused=int(hdr[native.SVQ_H_REFUSED]))


class ServiceWindowQuantiles:
    """A per-service, per-row percentile table.  Row 0 is before t0_ns, rows 1 .. n_windows are
    the windows, the last row is after them; a span is in the row of its finish time.  counts[class]:
    u64[n_services][rows]; values[measure][class]: u64[n_services][rows][n_q] in ns, 0 where the count is 0;
    header: the spans folded and refused."""

    def __init__(self, handler, q: Sequence[float], window_ns: int, n_windows: int, t0_ns: int, table: np.ndarray,
                 names: Sequence[str] = None):
        self.handler = handler
        self.q = tuple(q)
        self.window_ns, self.n_windows, self.t0_ns = int(window_ns), int(n_windows), int(t0_ns)
        self.names = names if names is not None else [s["name"] for s in handler.graph.canonical()["services"]]
        self.flat = np.ascontiguousarray(table, dtype=np.uint64).ravel()
        self.cells, self.header = decode_service_window_quantiles(self.flat, len(self.names), self.n_windows,
                                                                  len(self.q))
        self.counts = {c: self.cells[:, :, 0, k, 0] for k, c in enumerate(CLASS_NAMES)}
        self.values = {m: {c: self.cells[:, :, j, k, 1:] for k, c in enumerate(CLASS_NAMES)}
                       for j, m in enumerate(MEASURE_NAMES)}

    def _service(self, service) -> int:
        return self.names.index(service) if isinstance(service, str) else int(service)

    def series(self, service, measure: str, q: float, cls: str = "all") -> np.ndarray:
        """u64[n_windows + 2]: the value of `measure` at quantile q of one service (a name or an index), one
        per row; 0 where the row has no span in the class."""
        return self.values[measure][cls][self._service(service), :, self.q.index(q)]

    def _worst(self, measure, q, top, cls):
        col = self.values[measure][cls][:, :, self.q.index(q)].ravel()
        cnt = self.counts[cls].ravel()
        rows = self.n_windows + 2
        order = [i for i in _descending(col) if int(cnt[i])]
        return [(int(i // rows), int(i % rows), int(col[i])) for i in order[:top]]

    def worst(self, measure: str, q: float, top: int = 5, cls: str = "all") -> list:
        """[(service name, row, ns)]: the `top` cells with the largest value of `measure` at quantile q, among
        those that have a span in the class."""
        return [(self.names[s], r, v) for s, r, v in self._worst(measure, q, top, cls)]

    def to_text(self, top: int = None) -> str:
        """The cells by their largest-quantile duration, with each quantile of wait and duration."""
        h = self.header
        qs = [f"{f * 100:g}" for f in self.q]
        head = f"{'service':<24}{'row':>7}{'spans':>10}{'500s':>8}" + "".join(f"{'wait p' + x:>14}" for x in qs) \
            + "".join(f"{'dur p' + x:>14}" for x in qs)
        lines = [f"service window quantiles of {h['folded']} spans (ns), {self.n_windows} windows of {self.window_ns} ns"
                 + (f", {h['refused']} refused" if h["refused"] else ""), head]
        last = max(self.q)
        dur, wait = self.values["duration"]["all"], self.values["wait"]["all"]
        for s, r, _ in self._worst("duration", last, top, "all"):
            lines.append(f"{self.names[s]:<24}{r:>7}{int(self.counts['all'][s, r]):>10}{int(self.counts['500'][s, r]):>8}"
                         + "".join(f"{int(v):>14}" for v in wait[s, r]) + "".join(f"{int(v):>14}" for v in dur[s, r]))
        return "\n".join(lines)
