"""Per-service exact percentiles of queue wait, service time and duration.

    d = isim.DesHandler(handler, 300_000)                  # a DES on the item engine
    sq = d.service_quantiles(0, n, q=(0.5, 0.99, 0.999))   # the whole batch tapped, selected on the GPU
    print(sq.to_text(top=5))                               # the services with the largest p99.9 duration
    sq.worst("wait", 0.99, 3)                              # [(name, ns)] of the three largest p99 queue waits
    sq.values["duration"]["all"][s]                        # u64[n_q] of service s

The per-service view of service_request_duration_seconds: the spans of a
whole tapped batch (isim_serve_des_spans*, threshold 0) grouped by service,
and per service and class (all / 200 / 500) the nearest-rank order statistics
of S - a (wait), F - S (service) and F - a (duration).  The table is written,
not added into: order statistics do not merge across batches.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import native
from .des_spans import DES_SPAN_DTYPE
from .quantiles import CLASS_NAMES, DEFAULT_Q, _ppm_array, q_to_ppm

MEASURE_NAMES = ("wait", "service", "duration")  # native.SVQ_WAIT, SVQ_SERVICE, SVQ_DURATION
STAGE = native.SVQ_STAGE    # the device selects a service with at most this many spans in LDS
CHUNK = native.SVQ_CHUNK    # elements of a longer segment that one workgroup histograms per digit


def service_quantiles_table_words(handler, n_q: int) -> int:
    b = C.c_uint64()
    native.check(native.load().isim_service_quantiles_table_words(handler._h, n_q, C.byref(b)))
    return int(b.value)


def service_quantiles_workspace_bytes(handler, cap_spans: int, n_q: int) -> int:
    b = C.c_uint64()
    native.check(native.load().isim_service_quantiles_workspace_bytes(handler._h, cap_spans, n_q, C.byref(b)))
    return int(b.value)


def service_quantiles_device(handler, q: Sequence[float], d_off: int, d_spans: int, cap_spans: int, d_info: int,
                             d_out: int, d_workspace: int, workspace_bytes: int, stream: int = 0) -> None:
    """isim_service_quantiles_device over device addresses: selects over the spans a preceding
    serve_spans_device on the same stream wrote and writes d_out."""
    ppm = q_to_ppm(q)
    native.check(native.load().isim_service_quantiles_device(
        handler._h, _ppm_array(ppm), len(ppm), d_off or None, d_spans or None, cap_spans, d_info or None,
        d_out or None, d_workspace or None, workspace_bytes, stream or None))


def _table(handler, spans, q, device):
    spans = np.ascontiguousarray(spans, dtype=DES_SPAN_DTYPE)
    ppm = q_to_ppm(q)
    out = np.zeros(service_quantiles_table_words(handler, len(ppm)), np.uint64)
    sp = spans.ctypes.data if len(spans) else None
    lib = native.load()
    if device is None:
        native.check(lib.isim_service_quantiles_host(handler._h, _ppm_array(ppm), len(ppm), sp, len(spans),
                                                     out.ctypes.data))
    else:
        native.check(lib.isim_service_quantiles(device, handler._h, _ppm_array(ppm), len(ppm), sp, len(spans),
                                                out.ctypes.data))
    return out


def service_quantiles_host(handler, spans: np.ndarray, q: Sequence[float] = DEFAULT_Q) -> np.ndarray:
    """isim_service_quantiles_host: the table on the CPU over a DES_SPAN_DTYPE array; the flat u64 table."""
    return _table(handler, spans, q, None)


def service_quantiles(handler, spans: np.ndarray, q: Sequence[float] = DEFAULT_Q, device: int = 0) -> np.ndarray:
    """isim_service_quantiles: the same table on GPU `device`, host arrays in and out."""
    return _table(handler, spans, q, device)


def decode_service_quantiles(flat: np.ndarray, n_services: int, n_q: int):
    """The flat table as (cells u64[n_services][3 measures][3 classes][1 + n_q], {"folded", "refused"})."""
    flat = np.asarray(flat, dtype=np.uint64).ravel()
    H = native.SVQ_HEADER_WORDS
    assert flat.size == n_services * native.SVQ_MEASURES * native.SVQ_CLASSES * (1 + n_q) + H
    cells = flat[:-H].reshape(n_services, native.SVQ_MEASURES, native.SVQ_CLASSES, 1 + n_q)
    hdr = flat[-H:]
    return cells, dict(folded=int(hdr[native.SVQ_H_FOLDED]), refused=int(hdr[native.SVQ_H_REFUSED]))


def _descending(col: np.ndarray) -> np.ndarray:
    """The indices of a u64 column from its largest value down, equal values by index: exact for every u64."""
    return np.argsort(~np.asarray(col, dtype=np.uint64), kind="stable")


class ServiceQuantiles:
    """A per-service percentile table.  counts[class]: u64[n_services];
    values[measure][class]: u64[n_services][n_q] in ns, 0 where the count is 0; header: the spans folded and
    refused."""

    def __init__(self, handler, q: Sequence[float], table: np.ndarray, names: Sequence[str] = None):
        self.handler = handler
        self.q = tuple(q)
        self.names = names if names is not None else [s["name"] for s in handler.graph.canonical()["services"]]
        self.flat = np.ascontiguousarray(table, dtype=np.uint64).ravel()
        self.cells, self.header = decode_service_quantiles(self.flat, len(self.names), len(self.q))
        self.counts = {c: self.cells[:, 0, k, 0] for k, c in enumerate(CLASS_NAMES)}
        self.values = {m: {c: self.cells[:, j, k, 1:] for k, c in enumerate(CLASS_NAMES)}
                       for j, m in enumerate(MEASURE_NAMES)}

    def worst(self, measure: str, q: float, k: int = 5, cls: str = "all") -> list:
        """[(service name, ns)]: the k services with the largest value of `measure` at quantile q, among
        those that have a span in the class."""
        col = self.values[measure][cls][:, self.q.index(q)]
        order = [s for s in _descending(col) if int(self.counts[cls][s])]
        return [(self.names[s], int(col[s])) for s in order[:k]]

    def to_text(self, top: int = None) -> str:
        """The services by their largest-quantile duration, with each quantile of wait and duration."""
        h = self.header
        qs = [f"{f * 100:g}" for f in self.q]
        head = f"{'service':<24}{'spans':>10}{'500s':>8}" + "".join(f"{'wait p' + x:>14}" for x in qs) \
            + "".join(f"{'dur p' + x:>14}" for x in qs)
        lines = [f"service quantiles of {h['folded']} spans (ns)" + (f", {h['refused']} refused" if h["refused"] else ""),
                 head]
        last = max(range(len(self.q)), key=lambda i: self.q[i])
        dur, wait = self.values["duration"]["all"], self.values["wait"]["all"]
        order = [s for s in _descending(dur[:, last]) if int(self.counts["all"][s])]
        for s in order[:top]:
            lines.append(f"{self.names[s]:<24}{int(self.counts['all'][s]):>10}{int(self.counts['500'][s]):>8}"
                         + "".join(f"{int(v):>14}" for v in wait[s]) + "".join(f"{int(v):>14}" for v in dur[s]))
        return "\n".join(lines)
