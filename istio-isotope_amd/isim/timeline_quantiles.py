"""Per-window exact latency percentiles of a DES batch: p99 over time.

    t = isim.timeline_quantiles(arrivals, records, window_ns=10**9, n_windows=60)   # decoded dict
    t["latency_ns"][isim.native.Q_200, i, w]     # the i-th quantile of the 200s completing in window w
    isim.timeline_quantiles_device(...)          # device pointers + HIP stream, no host sync

For every row of the timeline (`isim.timeline`: what falls before ``t0_ns``,
the windows, what falls after the last) the exact order statistics of the
latencies that complete in it, per class (every record, the 200s, the 500s),
computed on the GPU through libisim (isim_timeline_quantiles*).  Quantiles are
fractions that are whole numbers of parts per million, ranks are nearest ranks
(`isim.quantile_rank`).  The table is written, not accumulated: to cover
several batches pass their concatenated arrivals and records.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import native
from .quantiles import DEFAULT_Q, _ppm_array, q_to_ppm
from .sim import REC_DTYPE


def timeline_quantiles_workspace_bytes(n: int, n_windows: int, n_q: int) -> int:
    b = C.c_uint64()
    native.check(native.load().isim_timeline_quantiles_workspace_bytes(n, n_windows, n_q, C.byref(b)))
    return int(b.value)


def timeline_quantiles_out_words(n_windows: int, n_q: int) -> int:
    """u64 words of the table: [n_windows + 2][3][1 + n_q] (rows before, the windows, after;
    per class the count, then the values)."""
    return (n_windows + 2) * 3 * (1 + n_q)


def timeline_quantiles_device(d_arrivals: int, d_records: int, n: int, window_ns: int, n_windows: int,
                              t0_ns: int = 0, q: Sequence[float] = DEFAULT_Q, *, d_out: int, d_workspace: int,
                              workspace_bytes: int = None, stream: int = 0) -> None:
    """Asynchronous on the current HIP device; pointers are device addresses.
    d_out: timeline_quantiles_out_words(n_windows, len(q)) u64, every word written;
    d_workspace: timeline_quantiles_workspace_bytes(n, n_windows, len(q)) bytes, dirty or not."""
    ppm = q_to_ppm(q)
    if workspace_bytes is None:
        workspace_bytes = timeline_quantiles_workspace_bytes(n, n_windows, len(ppm))
    p = native.TimelineParams(int(t0_ns), int(window_ns), int(n_windows), 0)
    native.check(native.load().isim_timeline_quantiles_device(
        d_arrivals or None, d_records or None, n, C.byref(p), _ppm_array(ppm), len(ppm), d_out or None,
        d_workspace or None, workspace_bytes, stream or None))


def timeline_quantiles_table(arrivals: np.ndarray, records: np.ndarray, window_ns: int, n_windows: int,
                             t0_ns: int = 0, q: Sequence[float] = DEFAULT_Q, device: int = 0) -> np.ndarray:
    """Synchronous: host arrays in (u64 arrivals, REC_DTYPE records), the raw u64 table out."""
    ppm = q_to_ppm(q)
    arr = np.ascontiguousarray(arrivals, dtype=np.uint64)
    recs = np.ascontiguousarray(records, dtype=REC_DTYPE)
    if len(arr) != len(recs):
        raise ValueError("arrivals and records differ in length")
    out = np.zeros(max(0, timeline_quantiles_out_words(n_windows, len(ppm))), np.uint64)
    p = native.TimelineParams(int(t0_ns), int(window_ns), int(n_windows), 0)
    native.check(native.load().isim_timeline_quantiles(
        device, arr.ctypes.data if len(arr) else None, recs.ctypes.data if len(recs) else None, len(arr), C.byref(p),
        _ppm_array(ppm), len(ppm), out.ctypes.data if out.size else None))
    return out


def decode_timeline_quantiles(out: np.ndarray, n_windows: int, t0_ns: int, window_ns: int, n_q: int) -> dict:
    """The table as per-window numpy arrays, in the style of decode_timeline:
    count[3][w] and latency_ns[3][n_q][w] (u64, class index native.Q_ALL / Q_200 / Q_500;
    latency_ns is 0 where count is 0), t_start_ns[w] (Python ints), and "before" / "after":
    count[3] and latency_ns[3][n_q] of the two outer rows."""
    t = np.asarray(out, dtype=np.uint64).reshape(n_windows + 2, 3, 1 + n_q)

    def fields(rows):
        return {"count": np.moveaxis(rows[..., 0], -1, 0).copy(),
                "latency_ns": np.moveaxis(np.moveaxis(rows[..., 1:], -1, 0), -1, 0).copy()}

    d = fields(t[1:-1])
    d["before"] = fields(t[0])
    d["after"] = fields(t[-1])
    d["t_start_ns"] = np.array([int(t0_ns) + w * int(window_ns) for w in range(n_windows)], dtype=object)
    return d


def timeline_quantiles(arrivals: np.ndarray, records: np.ndarray, window_ns: int, n_windows: int, t0_ns: int = 0,
                       q: Sequence[float] = DEFAULT_Q, device: int = 0) -> dict:
    """Synchronous: host arrays in, the decoded per-window quantiles out (plus "q": the fractions)."""
    q = tuple(q)
    d = decode_timeline_quantiles(timeline_quantiles_table(arrivals, records, window_ns, n_windows, t0_ns, q, device),
                                  n_windows, t0_ns, window_ns, len(q))
    d["q"] = q
    return d
