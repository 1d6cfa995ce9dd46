"""Load profiles for the DES: steps, spikes, pauses and paced arrivals.

    p = isim.LoadProfile.steps([(2 * 10**9, 6_000_000), (10**9, 600_000)], then_mean_ns=6_000_000)
    p = isim.LoadProfile.ramp(6_000_000, 600_000, 10 * 10**9, n_steps=50, then_mean_ns=600_000)
    p = isim.LoadProfile([(10**9, 1_000_000), (3 * 10**9, 0), (0, 1_000_000)], paced=True)   # a 3 s pause
    d = isim.DesHandler(handler, profile=p)            # serve, arrivals, timeline*, all under the profile
    a = isim.profile_arrivals(handler, p, trace_begin, n)

A profile is a list of (duration_ns, mean_interarrival_ns) segments; the last
runs forever and has duration 0; a mean of 0 is a pause.  Arrivals are a time
change of the unit-rate stream the constant-mean DES draws from (the same
Philox draws, no new randomness), or evenly paced (Fortio's default) with
``paced=True``.  The rule is exact integer arithmetic in libisim
(isim_load_profile_time on the host, isim_profile_arrivals* and
isim_serve_des_profile* on the GPU).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import native


class LoadProfile:
    def __init__(self, segments, paced: bool = False):
        self.segments = [(int(d), int(m)) for d, m in segments]
        self.paced = bool(paced)
        self._seg = (native.LoadSegment * max(1, len(self.segments)))(*[native.LoadSegment(d, m)
                                                                       for d, m in self.segments])
        # the C structure points into self._seg: both live as long as this object
        self._c = native.LoadProfile(C.cast(self._seg, C.POINTER(native.LoadSegment)), len(self.segments),
                                     native.LP_PACED if self.paced else 0)

    def __repr__(self) -> str:
        return f"LoadProfile({self.segments!r}, paced={self.paced})"

    @property
    def c(self):
        """byref of the isim_load_profile (valid while this object lives)."""
        return C.byref(self._c)

    @classmethod
    def constant(cls, mean_ns: int, paced: bool = False) -> "LoadProfile":
        return cls([(0, mean_ns)], paced)

    @classmethod
    def steps(cls, steps, then_mean_ns: int, paced: bool = False) -> "LoadProfile":
        """[(duration_ns, mean_ns), ...] in turn, then then_mean_ns forever."""
        return cls(list(steps) + [(0, then_mean_ns)], paced)

    @classmethod
    def ramp(cls, mean_from_ns: int, mean_to_ns: int, duration_ns: int, n_steps: int, then_mean_ns: int,
             paced: bool = False) -> "LoadProfile":
        """A staircase of n_steps equal-length segments over duration_ns whose RATE (1 / mean)
        goes linearly from 1 / mean_from_ns (first step) to 1 / mean_to_ns (last step), each
        mean rounded to the nearest ns; then then_mean_ns forever."""
        mf, mt, n = int(mean_from_ns), int(mean_to_ns), int(n_steps)
        if n < 2 or mf < 1 or mt < 1 or int(duration_ns) < n:
            raise ValueError("ramp needs n_steps >= 2, positive means and duration_ns >= n_steps")
        segs = []
        for k in range(n):
            # rate_k = ((n-1-k) / mf + k / mt) / (n-1)
            num, den = (n - 1) * mf * mt, (n - 1 - k) * mt + k * mf
            d = int(duration_ns) * (k + 1) // n - int(duration_ns) * k // n
            segs.append((d, (2 * num + den) // (2 * den)))
        return cls(segs + [(0, then_mean_ns)], paced)

    def time(self, work_q24: int) -> int:
        """t(u): the time (ns) at which work_q24 (Q24) of the unit-rate stream is done."""
        t = C.c_uint64()
        native.check(native.load().isim_load_profile_time(self.c, int(work_q24), C.byref(t)))
        return int(t.value)


def profile_arrivals_workspace_bytes(n: int) -> int:
    b = C.c_uint64()
    native.check(native.load().isim_profile_arrivals_workspace_bytes(n, C.byref(b)))
    return int(b.value)


def profile_arrivals(handler, profile: LoadProfile, trace_begin: int, n: int, device: int = 0) -> np.ndarray:
    """Synchronous: the arrival times (ns since batch start) of traces
    [trace_begin, trace_begin + n) under the profile, as a u64 array."""
    out = np.zeros(n, np.uint64)
    native.check(native.load().isim_profile_arrivals(handler._h, device, profile.c, trace_begin, n,
                                                     out.ctypes.data if n else None))
    return out


def profile_arrivals_device(handler, profile: LoadProfile, trace_begin: int, n: int, *, d_arrivals: int,
                            d_workspace: int, workspace_bytes: int = None, stream: int = 0) -> None:
    """Asynchronous on the current HIP device; pointers are device addresses.
    d_arrivals: n u64; d_workspace: profile_arrivals_workspace_bytes(n) bytes, dirty or not."""
    if workspace_bytes is None:
        workspace_bytes = profile_arrivals_workspace_bytes(n)
    native.check(native.load().isim_profile_arrivals_device(handler._h, profile.c, trace_begin, n,
                                                            d_arrivals or None, d_workspace or None,
                                                            workspace_bytes, stream or None))
