"""Exact latency percentiles from per-trace records.

    isim.latency_quantiles(records, q=(0.5, 0.75, 0.9, 0.99, 0.999))
        -> {"all": {"count": N, "q": {0.5: ns, ...}}, "200": ..., "500": ...}
    isim.latency_quantiles_device(d_records, n, q, d_out=..., d_workspace=..., stream=0)
        device pointers + HIP stream, no host sync (as Handler.serve_device)
    isim.quantile_rank(n, q_ppm)   — the nearest-rank rule, on the host

The Fortio client's latency report (p50 / p75 / p90 / p99 / p99.9) as exact
order statistics of ``latency_ns``: an MSD radix select on the GPU through
libisim (isim_latency_quantiles*), per class (every record, the 200s, the
500s).  Quantiles are fractions that are whole numbers of parts per million.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Sequence

import numpy as np

from . import native
from .sim import REC_DTYPE

DEFAULT_Q = (0.5, 0.75, 0.9, 0.99, 0.999)
CLASS_NAMES = ("all", "200", "500")  # native.Q_ALL, Q_200, Q_500


def q_to_ppm(q: Iterable[float]) -> list:
    """Fractions in [0, 1] to parts per million; a fraction that is not a
    whole number of ppm is rejected, not rounded."""
    out = []
    for f in q:
        ppm = round(float(f) * 1e6)
        if not 0 <= ppm <= 1_000_000 or abs(float(f) * 1e6 - ppm) > 1e-6:
            raise ValueError(f"quantile {f!r} is not a whole number of parts per million in [0, 1]")
        out.append(int(ppm))
    return out


def _ppm_array(ppm: Sequence[int]):
    return (C.c_uint32 * max(1, len(ppm)))(*ppm)


def quantile_rank(n: int, q_ppm: int) -> int:
    """isim_quantile_rank: the 1-based nearest rank max(1, ceil(q_ppm * n / 1e6))."""
    k = C.c_uint64()
    native.check(native.load().isim_quantile_rank(n, q_ppm, C.byref(k)))
    return int(k.value)


def quantiles_workspace_bytes(n_q: int) -> int:
    b = C.c_uint64()
    native.check(native.load().isim_quantiles_workspace_bytes(n_q, C.byref(b)))
    return int(b.value)


def quantiles_out_words(n_q: int) -> int:
    """u64 words of the output: [3][1 + n_q], per class the count then the values."""
    return 3 * (1 + n_q)


def latency_quantiles_device(d_records: int, n: int, q: Sequence[float] = DEFAULT_Q, *, d_out: int,
                             d_workspace: int, workspace_bytes: int = None, stream: int = 0) -> None:
    """Asynchronous on the current HIP device; pointers are device addresses.
    d_out: quantiles_out_words(len(q)) u64; d_workspace: quantiles_workspace_bytes(len(q))
    bytes (workspace_bytes: its size when it was allocated elsewhere), dirty or not."""
    ppm = q_to_ppm(q)
    if workspace_bytes is None:
        workspace_bytes = quantiles_workspace_bytes(len(ppm))
    native.check(native.load().isim_latency_quantiles_device(
        d_records or None, n, _ppm_array(ppm), len(ppm), d_out or None, d_workspace or None, workspace_bytes,
        stream or None))


def decode_quantiles(out: np.ndarray, q: Sequence[float]) -> dict:
    """The u64[3][1 + n_q] output as {"all" | "200" | "500": {"count": N, "q": {fraction: ns}}}."""
    out = np.asarray(out, dtype=np.uint64).reshape(3, 1 + len(q))
    return {name: {"count": int(out[c, 0]), "q": {f: int(out[c, 1 + i]) for i, f in enumerate(q)}}
            for c, name in enumerate(CLASS_NAMES)}


def latency_quantiles(records: np.ndarray, q: Sequence[float] = DEFAULT_Q, device: int = 0) -> dict:
    """Synchronous: a host REC_DTYPE array in, the decoded quantiles out."""
    q = tuple(q)
    ppm = q_to_ppm(q)
    recs = np.ascontiguousarray(records, dtype=REC_DTYPE)
    out = np.zeros(quantiles_out_words(len(ppm)), np.uint64)
    native.check(native.load().isim_latency_quantiles(
        device, recs.ctypes.data if len(recs) else None, len(recs), _ppm_array(ppm), len(ppm), out.ctypes.data))
    return decode_quantiles(out, q)
