"""The load-test timeline of a DES batch.

    a = isim.des_arrivals(handler, mean_interarrival_ns, trace_begin, n)      # u64 ns, the engine's own
    t = isim.timeline(a, records, window_ns=10**9, n_windows=60)              # decoded dict
    isim.des_arrivals_device(...) / isim.timeline_device(...)                 # device pointers, no host sync

Arrival times are the ones ``isim_serve_des*`` uses for the same seed, mean
and trace ids; the timeline bins arrivals and completions (arrival +
latency) into windows of simulated time on the GPU through libisim
(isim_des_arrivals*, isim_timeline*): per window the requests that arrived
and, of those that completed in it, by response code, their count, latency
sum, latency maximum and Prometheus histogram.  Row 0 collects what falls
before ``t0_ns``, the last row what falls after the last window.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import native
from .sim import REC_DTYPE


def _des_params(mean_interarrival_ns: int) -> native.DesParams:
    return native.DesParams(int(mean_interarrival_ns), 0, 0)


def des_arrivals_workspace_bytes(n: int) -> int:
    b = C.c_uint64()
    native.check(native.load().isim_des_arrivals_workspace_bytes(n, C.byref(b)))
    return int(b.value)


def des_arrivals(handler, mean_interarrival_ns: int, trace_begin: int, n: int, device: int = 0) -> np.ndarray:
    """Synchronous: the arrival times (ns since batch start) of traces
    [trace_begin, trace_begin + n), as a u64 array."""
    out = np.zeros(n, np.uint64)
    p = _des_params(mean_interarrival_ns)
    native.check(native.load().isim_des_arrivals(handler._h, device, C.byref(p), trace_begin, n,
                                                 out.ctypes.data if n else None))
    return out


def des_arrivals_device(handler, mean_interarrival_ns: int, trace_begin: int, n: int, *, d_arrivals: int,
                        d_workspace: int, workspace_bytes: int = None, stream: int = 0) -> None:
    """Asynchronous on the current HIP device; pointers are device addresses.
    d_arrivals: n u64; d_workspace: des_arrivals_workspace_bytes(n) bytes, dirty or not."""
    if workspace_bytes is None:
        workspace_bytes = des_arrivals_workspace_bytes(n)
    p = _des_params(mean_interarrival_ns)
    native.check(native.load().isim_des_arrivals_device(handler._h, C.byref(p), trace_begin, n, d_arrivals or None,
                                                        d_workspace or None, workspace_bytes, stream or None))


def timeline_out_words(n_windows: int) -> int:
    """u64 words of the table: [n_windows + 2][TL_ROW_WORDS] (rows before, the windows, after)."""
    return (n_windows + 2) * native.TL_ROW_WORDS


def timeline_device(d_arrivals: int, d_records: int, n: int, window_ns: int, n_windows: int, t0_ns: int = 0, *,
                    d_out: int, stream: int = 0) -> None:
    """Asynchronous on the current HIP device.  d_out (timeline_out_words(n_windows)
    u64) is accumulated into: zero it before the first call."""
    p = native.TimelineParams(int(t0_ns), int(window_ns), int(n_windows), 0)
    native.check(native.load().isim_timeline_device(d_arrivals or None, d_records or None, n, C.byref(p),
                                                    d_out or None, stream or None))


def timeline_merge(n_windows: int, dst: np.ndarray, src: np.ndarray) -> np.ndarray:
    """isim_timeline_merge on the host: dst += src (the maxima by max); returns dst."""
    src = np.ascontiguousarray(src, dtype=np.uint64)
    if dst.dtype != np.uint64 or not dst.flags.c_contiguous or dst.size != timeline_out_words(n_windows) \
            or src.size != dst.size:
        raise ValueError("timeline tables must be contiguous u64 arrays of timeline_out_words(n_windows)")
    native.check(native.load().isim_timeline_merge(n_windows, dst.ctypes.data, src.ctypes.data))
    return dst


def decode_timeline(out: np.ndarray, n_windows: int, t0_ns: int, window_ns: int) -> dict:
    """The table as per-window numpy arrays.  Integer fields are exact
    (u64; t_start_ns as Python ints, which do not overflow); throughput_per_s
    and mean_latency_ns are the stated float ratios (NaN where nothing completed).

    t_start_ns[w], arrived[w], done[2][w], sum_latency_ns[2][w], max_latency_ns[2][w],
    prom[2][33][w-major: prom[c, w, b]], in_flight_end[w] (requests arrived and not
    completed by the end of window w, the "before" row included),
    throughput_per_s[w] = (done[0] + done[1]) / window seconds,
    mean_latency_ns[2][w] = sum_latency_ns / done; "before" and "after": the
    same integer fields of the two outer rows."""
    W = native.TL_ROW_WORDS
    t = np.asarray(out, dtype=np.uint64).reshape(n_windows + 2, W)

    def fields(rows):
        return {
            "arrived": rows[..., native.TL_ARRIVED].copy(),
            "done": np.moveaxis(rows[..., native.TL_DONE:native.TL_DONE + 2], -1, 0).copy(),
            "sum_latency_ns": np.moveaxis(rows[..., native.TL_SUM_LAT:native.TL_SUM_LAT + 2], -1, 0).copy(),
            "max_latency_ns": np.moveaxis(rows[..., native.TL_MAX_LAT:native.TL_MAX_LAT + 2], -1, 0).copy(),
            "prom": np.moveaxis(rows[..., native.TL_PROM:].reshape(rows.shape[:-1] + (2, native.N_PROM)), -2, 0).copy(),
        }

    d = fields(t[1:-1])
    d["before"] = fields(t[0])
    d["after"] = fields(t[-1])
    d["t_start_ns"] = np.array([int(t0_ns) + w * int(window_ns) for w in range(n_windows)], dtype=object)
    done_all = d["done"][0] + d["done"][1]
    b = d["before"]
    # arrived - done stays >= 0 along the prefix (a completion never precedes its arrival), so u64 holds it
    d["in_flight_end"] = (np.cumsum(d["arrived"], dtype=np.uint64) + b["arrived"]
                          - np.cumsum(done_all, dtype=np.uint64) - (b["done"][0] + b["done"][1]))
    d["throughput_per_s"] = done_all.astype(np.float64) * (1e9 / float(window_ns))
    with np.errstate(divide="ignore", invalid="ignore"):
        d["mean_latency_ns"] = d["sum_latency_ns"].astype(np.float64) / d["done"].astype(np.float64)
    return d


def timeline(arrivals: np.ndarray, records: np.ndarray, window_ns: int, n_windows: int, t0_ns: int = 0,
             device: int = 0) -> dict:
    """Synchronous: host arrays in (u64 arrivals, REC_DTYPE records), the decoded timeline out."""
    return decode_timeline(timeline_table(arrivals, records, window_ns, n_windows, t0_ns, device), n_windows, t0_ns,
                           window_ns)


def timeline_table(arrivals: np.ndarray, records: np.ndarray, window_ns: int, n_windows: int, t0_ns: int = 0,
                   device: int = 0, out: np.ndarray = None) -> np.ndarray:
    """The raw u64 table of `timeline`; `out` (a table of the same shape) is accumulated into."""
    arr = np.ascontiguousarray(arrivals, dtype=np.uint64)
    recs = np.ascontiguousarray(records, dtype=REC_DTYPE)
    if len(arr) != len(recs):
        raise ValueError("arrivals and records differ in length")
    if out is None:
        out = np.zeros(max(0, timeline_out_words(n_windows)), np.uint64)
    p = native.TimelineParams(int(t0_ns), int(window_ns), int(n_windows), 0)
    native.check(native.load().isim_timeline(device, arr.ctypes.data if len(arr) else None,
                                             recs.ctypes.data if len(recs) else None, len(arr), C.byref(p),
                                             out.ctypes.data if out.size else None))
    return out
