"""Per-service latency sketch: percentiles across batches and GPUs.

    d = isim.DesHandler(handler, 300_000)              # a DES on the item engine
    sk = d.service_sketch(0, n, sub_bits=3)            # the whole batch tapped, sketched on the GPU
    d.service_sketch(n, n, into=sk)                    # the next batch adds into the same table
    sk.merge(other)                                    # or tables of other GPUs, on the host
    sk.worst("wait", 0.99, 3)                          # [(name, (lo, hi))] of the three largest p99 queue waits
    sk.quantiles((0.5, 0.99))["duration"]["all"]["hi"][s]   # u64[n_q] of service s

The mergeable counterpart of `isim.service_quantiles`: per service and measure
(wait S - a, service F - S, duration F - a) one log-linear table by code and
bin, the kind `isim.latency_sketch` fills.  Every word is a count, so tables
add over batches, shards and GPUs; a quantile comes back as a bracket
``[lo, hi]`` that contains the exact order statistic, with
``hi - lo < max(1, lo >> sub_bits)``.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import native
from .des_spans import DES_SPAN_DTYPE
from .quantiles import CLASS_NAMES, DEFAULT_Q, _ppm_array, q_to_ppm
from .service_quantiles import MEASURE_NAMES, _descending

DEFAULT_SUB_BITS = 3
SHORT = native.SVS_SHORT    # the device adds a service with at most this many spans straight into the table


def service_sketch_table_words(handler, sub_bits: int = DEFAULT_SUB_BITS) -> int:
    b = C.c_uint64()
    native.check(native.load().isim_service_sketch_table_words(handler._h, sub_bits, C.byref(b)))
    return int(b.value)


def service_sketch_workspace_bytes(handler, cap_spans: int) -> int:
    b = C.c_uint64()
    native.check(native.load().isim_service_sketch_workspace_bytes(handler._h, cap_spans, C.byref(b)))
    return int(b.value)


def service_sketch_device(handler, sub_bits: int, d_off: int, d_spans: int, cap_spans: int, d_info: int,
                          d_table: int, d_workspace: int, workspace_bytes: int, stream: int = 0) -> None:
    """isim_service_sketch_device over device addresses: adds the spans a preceding serve_spans_device on the
    same stream wrote into d_table (zero it before the first call)."""
    native.check(native.load().isim_service_sketch_device(
        handler._h, sub_bits, d_off or None, d_spans or None, cap_spans, d_info or None, d_table or None,
        d_workspace or None, workspace_bytes, stream or None))


def _table_ok(a, words: int) -> bool:
    return isinstance(a, np.ndarray) and a.dtype == np.uint64 and a.flags.c_contiguous and a.size == words


def _fold(handler, spans, sub_bits, out, device):
    spans = np.ascontiguousarray(spans, dtype=DES_SPAN_DTYPE)
    words = service_sketch_table_words(handler, sub_bits)
    if out is None:
        out = np.zeros(words, np.uint64)
    elif not _table_ok(out, words):
        raise ValueError("out must be a contiguous u64 array of service_sketch_table_words(handler, sub_bits)")
    sp = spans.ctypes.data if len(spans) else None
    lib = native.load()
    if device is None:
        native.check(lib.isim_service_sketch_host(handler._h, sub_bits, sp, len(spans), out.ctypes.data))
    else:
        native.check(lib.isim_service_sketch(device, handler._h, sub_bits, sp, len(spans), out.ctypes.data))
    return out


def service_sketch_host(handler, spans: np.ndarray, sub_bits: int = DEFAULT_SUB_BITS,
                        out: np.ndarray = None) -> np.ndarray:
    """isim_service_sketch_host: a DES_SPAN_DTYPE array folded on the CPU; the flat u64 table.  `out` (a
    table of the same handler and sub_bits) is accumulated into."""
    return _fold(handler, spans, sub_bits, out, None)


def service_sketch(handler, spans: np.ndarray, sub_bits: int = DEFAULT_SUB_BITS, device: int = 0,
                   out: np.ndarray = None) -> np.ndarray:
    """isim_service_sketch: the same fold on GPU `device`, host arrays in and out."""
    return _fold(handler, spans, sub_bits, out, device)


def service_sketch_merge(handler, sub_bits: int, dst: np.ndarray, src: np.ndarray) -> np.ndarray:
    """isim_service_sketch_merge on the host: dst += src, every word, the header included; returns dst."""
    words = service_sketch_table_words(handler, sub_bits)
    src = np.ascontiguousarray(src, dtype=np.uint64)
    if not _table_ok(dst, words) or src.size != words:
        raise ValueError("tables must be contiguous u64 arrays of service_sketch_table_words(handler, sub_bits)")
    native.check(native.load().isim_service_sketch_merge(handler._h, sub_bits, dst.ctypes.data, src.ctypes.data))
    return dst


def service_sketch_quantiles(handler, sub_bits: int, table: np.ndarray, q: Sequence[float] = DEFAULT_Q) -> np.ndarray:
    """isim_service_sketch_quantiles: u64[n_services][3 measures][3 classes][1 + 2 * n_q], per class the
    count, then lo and hi per quantile."""
    ppm = q_to_ppm(q)
    table = np.ascontiguousarray(table, dtype=np.uint64).ravel()
    if table.size != service_sketch_table_words(handler, sub_bits):
        raise ValueError("table must hold service_sketch_table_words(handler, sub_bits) words")
    n = (table.size - native.SVQ_HEADER_WORDS) // native.SK_WORDS(sub_bits)  # n_services * 3
    out = np.zeros(max(1, n * native.SKQ_OUT_WORDS(max(1, len(ppm)))), np.uint64)
    native.check(native.load().isim_service_sketch_quantiles(handler._h, sub_bits, table.ctypes.data, _ppm_array(ppm),
                                                             len(ppm), out.ctypes.data))
    return out[:n * native.SKQ_OUT_WORDS(len(ppm))].reshape(n // native.SVQ_MEASURES, native.SVQ_MEASURES, 3,
                                                            1 + 2 * len(ppm))


class ServiceSketch:
    """A per-service sketch table of `handler` at `sub_bits`.  flat: the u64 table, zeros
    unless given; blocks: its view u64[n_services][3 measures][2 codes][bins]; header: the spans folded and
    refused over everything added so far."""

    def __init__(self, handler, sub_bits: int = DEFAULT_SUB_BITS, flat: np.ndarray = None,
                 names: Sequence[str] = None):
        self.handler = handler
        self.sub_bits = int(sub_bits)
        self.names = list(names) if names is not None else [s["name"] for s in handler.graph.canonical()["services"]]
        words = service_sketch_table_words(handler, self.sub_bits)
        if len(self.names) * native.SVQ_MEASURES * native.SK_WORDS(self.sub_bits) + native.SVQ_HEADER_WORDS != words:
            raise ValueError("names must hold one name per service of the handler")
        self.flat = np.zeros(words, np.uint64) if flat is None else np.ascontiguousarray(flat, dtype=np.uint64).ravel()
        if self.flat.size != words:
            raise ValueError("flat must hold service_sketch_table_words(handler, sub_bits) words")
        H = native.SVQ_HEADER_WORDS
        self.blocks = self.flat[:-H].reshape(len(self.names), native.SVQ_MEASURES, 2, native.SK_BINS(self.sub_bits))

    @property
    def header(self) -> dict:
        hdr = self.flat[-native.SVQ_HEADER_WORDS:]
        return dict(folded=int(hdr[native.SVQ_H_FOLDED]), refused=int(hdr[native.SVQ_H_REFUSED]))

    def add_spans(self, spans: np.ndarray, device: int = 0) -> "ServiceSketch":
        """Adds a DES_SPAN_DTYPE array on GPU `device` (None: on the CPU)."""
        _fold(self.handler, spans, self.sub_bits, self.flat, device)
        return self

    def merge(self, other: "ServiceSketch") -> "ServiceSketch":
        """self += other (the same handler's services and sub_bits), header included; returns self."""
        if other.sub_bits != self.sub_bits or other.flat.size != self.flat.size:
            raise ValueError("sketches of different sub_bits or services do not merge")
        service_sketch_merge(self.handler, self.sub_bits, self.flat, other.flat)
        return self

    def quantiles(self, q: Sequence[float] = DEFAULT_Q) -> dict:
        """{measure: {class: {"count": u64[n_services], "lo": u64[n_services][n_q], "hi": the same}}}: the
        exact order statistic of everything added lies in [lo, hi]; both 0 where the count is 0."""
        q = tuple(q)
        out = service_sketch_quantiles(self.handler, self.sub_bits, self.flat, q)
        return {m: {c: {"count": out[:, j, k, 0], "lo": out[:, j, k, 1::2], "hi": out[:, j, k, 2::2]}
                    for k, c in enumerate(CLASS_NAMES)} for j, m in enumerate(MEASURE_NAMES)}

    def worst(self, measure: str, q: float, k: int = 5, cls: str = "all") -> list:
        """[(service name, (lo, hi))]: the k services with the largest bracket of `measure` at quantile q,
        ordered by hi, among those that have a span in the class."""
        d = self.quantiles((q,))[measure][cls]
        order = [s for s in _descending(d["hi"][:, 0]) if int(d["count"][s])]
        return [(self.names[s], (int(d["lo"][s, 0]), int(d["hi"][s, 0]))) for s in order[:k]]

    def to_text(self, q: Sequence[float] = DEFAULT_Q, top: int = None) -> str:
        """The services by the hi of their largest-quantile duration, with each quantile's bracket of wait
        and duration."""
        q = tuple(q)
        h = self.header
        qs = [f"{f * 100:g}" for f in q]
        head = f"{'service':<24}{'spans':>10}{'500s':>8}" + "".join(f"{'wait p' + x:>26}" for x in qs) \
            + "".join(f"{'dur p' + x:>26}" for x in qs)
        lines = [f"service sketch of {h['folded']} spans (ns, sub_bits {self.sub_bits})"
                 + (f", {h['refused']} refused" if h["refused"] else ""), head]
        d = self.quantiles(q)
        dur, wait = d["duration"]["all"], d["wait"]["all"]
        last = max(range(len(q)), key=lambda i: q[i])
        order = [s for s in _descending(dur["hi"][:, last]) if int(dur["count"][s])]
        br = lambda x, s, i: f"{int(x['lo'][s, i])}..{int(x['hi'][s, i])}"  # noqa: E731
        for s in order[:top]:
            lines.append(f"{self.names[s]:<24}{int(dur['count'][s]):>10}{int(d['duration']['500']['count'][s]):>8}"
                         + "".join(f"{br(wait, s, i):>26}" for i in range(len(q)))
                         + "".join(f"{br(dur, s, i):>26}" for i in range(len(q))))
        return "\n".join(lines)
