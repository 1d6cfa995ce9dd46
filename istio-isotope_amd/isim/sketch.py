"""Mergeable latency sketch: percentiles across batches, shards and GPUs.

    t = isim.latency_sketch(records, sub_bits=7)                 # u64[2][bins], by code and bin
    isim.latency_sketch(more_records, sub_bits=7, out=t)         # accumulates: two batches, one table
    isim.sketch_merge(7, t, other)                               # or merge tables on the host
    isim.sketch_quantiles(7, t)["all"]["q"][0.99]                # (lo, hi): a bracket around the exact p99
    isim.timeline_sketch(arrivals, records, 10**9, 60)           # one table per window, decoded brackets
    isim.latency_sketch_device(...) / isim.timeline_sketch_device(...)   # device pointers, no host sync

A log-linear histogram of ``latency_ns`` (the HdrHistogram / Fortio kind),
filled on the GPU through libisim (isim_latency_sketch*, isim_timeline_sketch*).
Every word is a count and merges by addition, so a table folds over batches,
shards and GPUs (a SUM all-reduce of the raw words) where the exact selects
(`isim.latency_quantiles`, `isim.timeline_quantiles`) need every record in one
buffer.  A quantile comes back as a bracket ``[lo, hi]`` that contains the exact
order statistic, with ``hi - lo < max(1, lo >> sub_bits)``.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import native
from .quantiles import CLASS_NAMES, DEFAULT_Q, _ppm_array, q_to_ppm
from .sim import REC_DTYPE

DEFAULT_SUB_BITS = 7


def sketch_bins(sub_bits: int) -> int:
    """ISIM_SK_BINS: bins per code, (65 - s) << s."""
    if not 0 <= sub_bits <= native.SK_MAX_SUB_BITS:
        raise ValueError("sub_bits must be 0..7")
    return native.SK_BINS(sub_bits)


def sketch_words(sub_bits: int) -> int:
    """ISIM_SK_WORDS: u64 words of one table, [2][bins]."""
    return 2 * sketch_bins(sub_bits)


def sketch_bucket(sub_bits: int, v: int) -> int:
    """isim_sketch_bucket: the bin of a u64 latency."""
    b = C.c_uint32()
    native.check(native.load().isim_sketch_bucket(sub_bits, v, C.byref(b)))
    return int(b.value)


def sketch_bounds(sub_bits: int, bin: int) -> tuple:
    """isim_sketch_bounds: (lo, hi), the least and the greatest latency of a bin."""
    lo, hi = C.c_uint64(), C.c_uint64()
    native.check(native.load().isim_sketch_bounds(sub_bits, bin, C.byref(lo), C.byref(hi)))
    return int(lo.value), int(hi.value)


def _table_ok(a: np.ndarray, words: int) -> bool:
    return isinstance(a, np.ndarray) and a.dtype == np.uint64 and a.flags.c_contiguous and a.size == words


def sketch_merge(sub_bits: int, dst: np.ndarray, src: np.ndarray) -> np.ndarray:
    """isim_sketch_merge on the host: dst += src, for one table or a per-window stack of them; returns dst."""
    src = np.ascontiguousarray(src, dtype=np.uint64)
    words = sketch_words(sub_bits)
    if not isinstance(dst, np.ndarray) or not _table_ok(dst, dst.size) or dst.size == 0 or dst.size % words \
            or src.size != dst.size:
        raise ValueError("sketch tables must be contiguous u64 arrays of a whole number of sketch_words(sub_bits)")
    native.check(native.load().isim_sketch_merge(sub_bits, dst.size // words, dst.ctypes.data, src.ctypes.data))
    return dst


def sketch_quantiles(sub_bits: int, table: np.ndarray, q: Sequence[float] = DEFAULT_Q) -> dict:
    """isim_sketch_quantiles of one table: {"all" | "200" | "500": {"count": N, "q": {fraction: (lo, hi)}}},
    each bracket containing the exact order statistic ((0, 0) for an empty class)."""
    q = tuple(q)
    ppm = q_to_ppm(q)
    table = np.ascontiguousarray(table, dtype=np.uint64)
    if table.size != sketch_words(sub_bits):
        raise ValueError("table must hold sketch_words(sub_bits) words")
    out = np.zeros(native.SKQ_OUT_WORDS(max(1, len(ppm))), np.uint64)
    native.check(native.load().isim_sketch_quantiles(sub_bits, table.ctypes.data, _ppm_array(ppm), len(ppm),
                                                     out.ctypes.data))
    out = out.reshape(3, -1)
    return {name: {"count": int(out[c, 0]),
                   "q": {f: (int(out[c, 1 + 2 * i]), int(out[c, 2 + 2 * i])) for i, f in enumerate(q)}}
            for c, name in enumerate(CLASS_NAMES)}


def latency_sketch_device(d_records: int, n: int, sub_bits: int = DEFAULT_SUB_BITS, *, d_table: int,
                          stream: int = 0) -> None:
    """Asynchronous on the current HIP device; pointers are device addresses.  d_table
    (sketch_words(sub_bits) u64) is accumulated into: zero it before the first call."""
    native.check(native.load().isim_latency_sketch_device(d_records or None, n, sub_bits, d_table or None,
                                                          stream or None))


def latency_sketch(records: np.ndarray, sub_bits: int = DEFAULT_SUB_BITS, device: int = 0,
                   out: np.ndarray = None) -> np.ndarray:
    """Synchronous: a host REC_DTYPE array in, the u64[2][bins] table out; `out` (a table of
    the same sub_bits) is accumulated into."""
    recs = np.ascontiguousarray(records, dtype=REC_DTYPE)
    words = sketch_words(sub_bits)
    if out is None:
        out = np.zeros(words, np.uint64)
    elif not _table_ok(out, words):
        raise ValueError("out must be a contiguous u64 array of sketch_words(sub_bits)")
    native.check(native.load().isim_latency_sketch(device, recs.ctypes.data if len(recs) else None, len(recs),
                                                   sub_bits, out.ctypes.data))
    return out


def timeline_sketch_out_words(n_windows: int, sub_bits: int) -> int:
    """ISIM_TLS_OUT_WORDS: u64 words of the per-window table, [n_windows + 2][2][bins]."""
    return (n_windows + 2) * sketch_words(sub_bits)


def timeline_sketch_device(d_arrivals: int, d_records: int, n: int, window_ns: int, n_windows: int, t0_ns: int = 0,
                           sub_bits: int = DEFAULT_SUB_BITS, *, d_out: int, stream: int = 0) -> None:
    """Asynchronous on the current HIP device.  d_out (timeline_sketch_out_words(n_windows,
    sub_bits) u64) is accumulated into: zero it before the first call."""
    p = native.TimelineParams(int(t0_ns), int(window_ns), int(n_windows), 0)
    native.check(native.load().isim_timeline_sketch_device(d_arrivals or None, d_records or None, n, C.byref(p),
                                                           sub_bits, d_out or None, stream or None))


def timeline_sketch_table(arrivals: np.ndarray, records: np.ndarray, window_ns: int, n_windows: int, t0_ns: int = 0,
                          sub_bits: int = DEFAULT_SUB_BITS, device: int = 0, out: np.ndarray = None) -> np.ndarray:
    """Synchronous: host arrays in (u64 arrivals, REC_DTYPE records), the raw u64 table out;
    `out` (a table of the same shape) is accumulated into."""
    arr = np.ascontiguousarray(arrivals, dtype=np.uint64)
    recs = np.ascontiguousarray(records, dtype=REC_DTYPE)
    if len(arr) != len(recs):
        raise ValueError("arrivals and records differ in length")
    sketch_bins(sub_bits)
    if out is None:
        out = np.zeros(max(0, timeline_sketch_out_words(n_windows, sub_bits)), np.uint64)
    elif not _table_ok(out, timeline_sketch_out_words(n_windows, sub_bits)):
        raise ValueError("out must be a contiguous u64 array of timeline_sketch_out_words(n_windows, sub_bits)")
    p = native.TimelineParams(int(t0_ns), int(window_ns), int(n_windows), 0)
    native.check(native.load().isim_timeline_sketch(device, arr.ctypes.data if len(arr) else None,
                                                    recs.ctypes.data if len(recs) else None, len(arr), C.byref(p),
                                                    sub_bits, out.ctypes.data if out.size else None))
    return out


def decode_timeline_sketch(out: np.ndarray, n_windows: int, t0_ns: int, window_ns: int, sub_bits: int,
                           q: Sequence[float] = DEFAULT_Q) -> dict:
    """The per-window table as per-row brackets, in the style of decode_timeline_quantiles:
    count[3][w], lo_ns[3][n_q][w] and hi_ns[3][n_q][w] (u64, class index native.Q_ALL / Q_200 /
    Q_500; the exact quantile of the records completing in window w lies in [lo_ns, hi_ns];
    both 0 where count is 0), t_start_ns[w] (Python ints), "before" / "after": count[3],
    lo_ns[3][n_q] and hi_ns[3][n_q] of the two outer rows, and "q": the fractions."""
    q = tuple(q)
    ppm = q_to_ppm(q)
    n_q = len(ppm)
    words = sketch_words(sub_bits)
    t = np.ascontiguousarray(out, dtype=np.uint64).reshape(n_windows + 2, words)
    rows = np.zeros((n_windows + 2, 3, native.SKQ_OUT_WORDS(max(1, n_q)) // 3), np.uint64)
    lib, qa = native.load(), _ppm_array(ppm)
    for r in range(n_windows + 2):
        if t[r].any():  # an empty row keeps its zeros
            native.check(lib.isim_sketch_quantiles(sub_bits, t[r].ctypes.data, qa, n_q, rows[r].ctypes.data))

    def fields(x):
        return {"count": np.moveaxis(x[..., 0], -1, 0).copy(),
                "lo_ns": np.moveaxis(np.moveaxis(x[..., 1:1 + 2 * n_q:2], -1, 0), -1, 0).copy(),
                "hi_ns": np.moveaxis(np.moveaxis(x[..., 2:2 + 2 * n_q:2], -1, 0), -1, 0).copy()}

    d = fields(rows[1:-1])
    d["before"] = fields(rows[0])
    d["after"] = fields(rows[-1])
    d["t_start_ns"] = np.array([int(t0_ns) + w * int(window_ns) for w in range(n_windows)], dtype=object)
    d["q"] = q
    return d


def timeline_sketch(arrivals: np.ndarray, records: np.ndarray, window_ns: int, n_windows: int, t0_ns: int = 0,
                    sub_bits: int = DEFAULT_SUB_BITS, q: Sequence[float] = DEFAULT_Q, device: int = 0) -> dict:
    """Synchronous: host arrays in, the decoded per-window brackets out, plus "table": the raw
    mergeable table (timeline_sketch_table)."""
    q_to_ppm(q)  # a bad fraction is rejected before the GPU runs
    table = timeline_sketch_table(arrivals, records, window_ns, n_windows, t0_ns, sub_bits, device)
    d = decode_timeline_sketch(table, n_windows, t0_ns, window_ns, sub_bits, q)
    d["table"] = table
    return d
