"""Load profiles on the CPU: the header's declarations, the
host map isim_load_profile_time against a big-integer restatement of the rule,
every argument the entry points reject (all on the host, before any HIP call)
and the Python builders."""
import bisect
import ctypes as C
import json
import os
import random
import re

import pytest

import isim
from isim import native

from conftest import ROOT

HDR = open(os.path.join(ROOT, "include", "isim.h")).read()
Q = 1 << 24
WORK_END = 1 << 63
FUNCS = ("isim_load_profile_time", "isim_profile_arrivals_workspace_bytes", "isim_profile_arrivals_device",
         "isim_profile_arrivals", "isim_serve_des_profile_device", "isim_serve_des_profile")


# ---- the rule in Python integers
def compile_profile(segs):
    """[(T_j, C_j, m_j)] and the list of C_{j+1} / T_{j+1} a segment ends at (None for the last)."""
    T = Cw = 0
    out, ends = [], []
    for j, (D, m) in enumerate(segs):
        out.append((T, Cw, m))
        if j + 1 < len(segs):
            W = (D << 24) // m if m else 0
            Cw = min(Cw + W, WORK_END)
            T += D
            ends.append((Cw, T))
        else:
            ends.append(None)
    return out, ends


def time_of(tab, u, cs=None):
    j = bisect.bisect_right(cs or [s[1] for s in tab], u) - 1      # the largest index with C_j <= u
    T, Cw, m = tab[j]
    return T + (((u - Cw) * m) >> 24)


def random_profile(rng, K):
    segs = []
    for j in range(K):
        kind = rng.random()
        if kind < 0.15:
            m = 0
        elif kind < 0.3:
            m = rng.choice([1, 2, 1 << 34, (1 << 34) - 1])
        else:
            m = int(2 ** rng.uniform(0, 34))
        D = rng.choice([1, 1 << 48, 10 ** 6]) if rng.random() < 0.2 else int(2 ** rng.uniform(0, 40 if K > 7 else 48))
        segs.append((max(1, D), m))
    segs[-1] = (0, max(1, segs[-1][1]))
    return segs


def c_time(p, u):
    t = C.c_uint64()
    rc = native.load().isim_load_profile_time(p.c, u, C.byref(t))
    return rc, int(t.value)


# ---- declarations
def test_header_and_bindings():
    assert re.search(r"#define\s+ISIM_LP_MAX_SEGMENTS\s+1024u", HDR) and native.LP_MAX_SEGMENTS == 1024
    assert re.search(r"#define\s+ISIM_LP_PACED\s+1u", HDR) and native.LP_PACED == 1
    assert re.search(r"typedef struct \{[^}]*duration_ns[^}]*mean_interarrival_ns[^}]*\} isim_load_segment;", HDR)
    assert re.search(r"typedef struct \{[^}]*segments;[^}]*n_segments;[^}]*flags;[^}]*\} isim_load_profile;", HDR)
    assert C.sizeof(native.LoadSegment) == 16 and C.sizeof(native.LoadProfile) == 16
    lib = native.load()
    for fn in FUNCS:
        assert re.search(r"ISIM_API int %s\(" % fn, HDR), fn
        assert fn in native.SIGNATURES and hasattr(lib, fn), fn
    assert re.search(r"#define\s+ISIM_ABI_VERSION\s+10\b", HDR) and lib.isim_abi_version() == 10


# ---- the host map
@pytest.mark.parametrize("K", [1, 2, 7, 1024])
def test_time_against_restatement(K):
    rng = random.Random(1000 + K)
    for trial in range(50):     # 4 x 50 = 200 profiles
        segs = random_profile(rng, K)
        p = isim.LoadProfile(segs)
        tab, ends = compile_profile(segs)
        cs = [s[1] for s in tab]
        pts = {0}
        for (T, Cw, m), end in zip(tab, ends):
            pts.update((Cw - 1, Cw, Cw + 1))
            if end is not None and end[0] > Cw:
                # the last work of a segment does not pass the segment's end
                assert time_of(tab, end[0] - 1, cs) <= end[1]
        pts.update(rng.randrange(0, max(2, 2 * tab[-1][1] + Q)) for _ in range(20 if K > 7 else 60))
        pts.update(int(2 ** rng.uniform(0, 63)) for _ in range(10))
        last = -1
        for u in sorted(x for x in pts if 0 <= x < WORK_END):
            want = time_of(tab, u, cs)
            rc, got = c_time(p, u)
            if want >= WORK_END:
                assert rc == native.ERANGE, (segs, u)
                continue
            assert rc == native.OK and got == want, (trial, u, got, want)
            assert got >= last, (trial, u)
            last = got


def test_time_edges():
    # a segment without work (D = 1 at a mean of 2^34: W = floor(2^24 / 2^34) = 0) is skipped, its duration counts
    p = isim.LoadProfile([(1000, 10), (1, 1 << 34), (0, 10)])
    c1 = (1000 << 24) // 10
    assert p.time(c1 - 1) <= 1000 and p.time(c1) == 1001 and p.time(c1 + Q) == 1011
    # so is a pause
    p = isim.LoadProfile([(1000, 10), (5_000_000_000, 0), (0, 10)])
    assert p.time(c1 - 1) <= 1000 and p.time(c1) == 1000 + 5_000_000_000
    # one paced unit of work per mean
    assert isim.LoadProfile.constant(12345).time(7 * Q) == 7 * 12345
    # C saturates at 2^63: 2^48 ns at a mean of 1 ns is 2^72 of work; the next segments are never reached
    p = isim.LoadProfile([(1 << 48, 1), (1 << 48, 1), (0, 1 << 34)])
    assert p.time(WORK_END - 1) == (WORK_END - 1) >> 24
    rc, _ = c_time(p, WORK_END)
    assert rc == native.ERANGE
    rc, _ = c_time(p, (1 << 64) - 1)
    assert rc == native.ERANGE
    # t would pass 2^63: u 2^34 / 2^24 with u near 2^62
    p = isim.LoadProfile.constant(1 << 34)
    assert c_time(p, 1 << 62)[0] == native.ERANGE
    assert c_time(p, (1 << 53) - 1) == (native.OK, (((1 << 53) - 1) << 34) >> 24)
    assert c_time(p, 1 << 53)[0] == native.ERANGE          # t = 2^63 exactly
    assert native.load().isim_load_profile_time(p.c, 0, None) == native.EINVAL


# ---- rejected arguments
def _raw(segs, n=None, flags=0, null_segments=False):
    arr = (native.LoadSegment * max(1, len(segs)))(*[native.LoadSegment(d, m) for d, m in segs])
    ptr = None if null_segments else C.cast(arr, C.POINTER(native.LoadSegment))
    lp = native.LoadProfile(ptr, len(segs) if n is None else n, flags)
    lp._keep = arr
    return lp


BAD_PROFILES = {
    "null segments": _raw([(0, 5)], null_segments=True),
    "no segments": _raw([(0, 5)], n=0),
    "too many segments": _raw([(1, 5)] * 1024 + [(0, 5)]),
    "unknown flag": _raw([(0, 5)], flags=2),
    "unknown flags": _raw([(0, 5)], flags=0x80000001),
    "zero duration inside": _raw([(0, 5), (0, 5)]),
    "duration above 2^48": _raw([((1 << 48) + 1, 5), (0, 5)]),
    "mean above 2^34": _raw([(10, (1 << 34) + 1), (0, 5)]),
    "last mean above 2^34": _raw([(0, (1 << 34) + 1)]),
    "nonzero last duration": _raw([(10, 5), (7, 5)]),
    "pause last": _raw([(10, 5), (0, 0)]),
}
GOOD = _raw([(1000, 5), (2000, 0), (0, 7)], flags=native.LP_PACED)


def _handler(doc=None):
    doc = doc or {"services": [{"name": "a", "isEntrypoint": True, "script": [{"sleep": "1ms"}]}]}
    return isim.Handler(isim.ServiceGraph.from_json(json.dumps(doc)), None, isim.SimParams())


def test_bad_profiles_host_function():
    lib, t = native.load(), C.c_uint64()
    assert lib.isim_load_profile_time(None, 0, C.byref(t)) == native.EINVAL
    for name, lp in BAD_PROFILES.items():
        assert lib.isim_load_profile_time(C.byref(lp), 0, C.byref(t)) == native.EINVAL, name
        assert "load profile" in native.last_error(), name
    assert lib.isim_load_profile_time(C.byref(GOOD), 0, C.byref(t)) == native.OK
    # the largest legal values pass
    assert lib.isim_load_profile_time(C.byref(_raw([(1 << 48, 1 << 34)] * 1023 + [(0, 1 << 34)])), 0,
                                      C.byref(t)) == native.OK


def test_arrivals_einval():
    """Fake device addresses: a call that got past the checks would fail with another status."""
    lib, h = native.load(), _handler()
    buf, ws, wsb = 0x10000, 0x20000, isim.profile_arrivals_workspace_bytes(100)

    def dev(hh=h._h, lp=GOOD, n=100, a=buf, w=ws, b=wsb):
        return lib.isim_profile_arrivals_device(hh, C.byref(lp) if lp is not None else None, 0, n, a, w, b, None)

    def host(hh=h._h, lp=GOOD, n=100, a=buf):
        return lib.isim_profile_arrivals(hh, 0, C.byref(lp) if lp is not None else None, 0, n, a)

    for f in (dev, host):
        assert f(hh=None) == native.EINVAL
        assert f(lp=None) == native.EINVAL
        assert f(a=None) == native.EINVAL
        for name, lp in BAD_PROFILES.items():
            assert f(lp=lp) == native.EINVAL, name
            assert f(lp=lp, n=0, a=None) == native.EINVAL, name      # a bad profile is bad with nothing to do, too
        assert f(n=(1 << 32) + 1) == native.EINVAL
        # the horizon: 2^32 traces at a mean of 2^34 ns reach 2^32 x 16.6 x 2^34 > 2^62
        assert f(lp=_raw([(0, 1 << 34)]), n=1 << 32) == native.EINVAL
        assert "horizon" in native.last_error()
        assert f(n=0, a=None) == native.OK
    assert dev(w=None) == native.EINVAL
    assert dev(b=wsb - 1) == native.EINVAL
    assert dev(b=0) == native.EINVAL
    assert "workspace" in native.last_error()
    assert dev(a=buf + 4) == native.EINVAL
    assert dev(w=ws + 4) == native.EINVAL
    assert "aligned" in native.last_error()


def test_arrivals_workspace_bytes():
    prev = 0
    for n in (0, 1, 8191, 8192, 8193, 1 << 24, 1 << 32):
        b = isim.profile_arrivals_workspace_bytes(n)
        # the chunk sums and a table of ISIM_LP_MAX_SEGMENTS compiled segments (24 B each)
        assert b >= prev and b >= 8 * ((n + 8191) // 8192 + 1) + 24 * 1024, n
        prev = b
    with pytest.raises(isim.IsimError) as e:
        isim.profile_arrivals_workspace_bytes((1 << 32) + 1)
    assert e.value.status == "EINVAL"
    assert native.load().isim_profile_arrivals_workspace_bytes(1, None) == native.EINVAL


def test_serve_des_profile_einval():
    lib, h = native.load(), _handler()
    d = isim.DesHandler(h, profile=isim.LoadProfile.constant(1000))
    rec, st, tab, ws = 0x10000, 0x20000, 0x30000, 0x40000
    wsb = d.workspace_bytes(100)

    def dev(hh=h._h, lp=GOOD, fl=0, n=100, r=rec, s=st, t=tab, w=ws, b=wsb):
        return lib.isim_serve_des_profile_device(hh, C.byref(lp) if lp is not None else None, fl, 0, n, r, s, t, w,
                                                 b, None)

    def host(hh=h._h, lp=GOOD, n=100):
        return lib.isim_serve_des_profile(hh, 0, C.byref(lp) if lp is not None else None, 0, n, None, None, None)

    for f in (dev, host):
        assert f(hh=None) == native.EINVAL
        assert f(lp=None) == native.EINVAL
        for name, lp in BAD_PROFILES.items():
            assert f(lp=lp) == native.EINVAL, name
        assert f(n=(1 << 31) + 1) == native.EINVAL
        assert f(lp=_raw([(0, 1 << 34)]), n=1 << 31) == native.EINVAL
        assert "horizon" in native.last_error()
    assert dev(fl=2) == native.EINVAL and dev(fl=3) == native.EINVAL
    assert dev(s=None) == native.EINVAL and dev(t=None) == native.EINVAL
    assert dev(n=0) == native.OK
    assert dev(w=None) == native.EINVAL
    assert dev(b=wsb - 1) == native.EINVAL
    assert "workspace" in native.last_error()
    for kw in ({"s": st + 4}, {"t": tab + 4}, {"w": ws + 4}, {"r": rec + 8}):
        assert dev(**kw) == native.EINVAL, kw
        assert "aligned" in native.last_error()
    # a graph outside the DES class is refused with the class's reason, as isim_serve_des* does
    out = {"services": [{"name": "a", "isEntrypoint": True, "numReplicas": 70000, "script": [{"sleep": "1ms"}]}]}
    ho = _handler(out)
    with pytest.raises(isim.IsimError):
        isim.DesHandler(ho, 1000)
    assert dev(hh=ho._h) == native.EINVAL


# ---- the builders
def test_builders():
    assert isim.LoadProfile.constant(6_000_000).segments == [(0, 6_000_000)]
    p = isim.LoadProfile.steps([(10 ** 9, 5_000_000), (2 * 10 ** 9, 0)], 7_000_000, paced=True)
    assert p.segments == [(10 ** 9, 5_000_000), (2 * 10 ** 9, 0), (0, 7_000_000)] and p.paced
    assert p.segments[-1][0] == 0
    assert p.time(0) == 0
    r = isim.LoadProfile.ramp(6_000_000, 600_000, 10 ** 10 + 3, 10, 600_000)
    assert len(r.segments) == 11 and r.segments[-1] == (0, 600_000)
    assert sum(d for d, _ in r.segments) == 10 ** 10 + 3
    assert r.segments[0][1] == 6_000_000 and r.segments[9][1] == 600_000
    # linear in rate: each step's rate is within the rounding of its mean (half a ns) of the line
    for k, (_, m) in enumerate(r.segments[:10]):
        rate = ((9 - k) / 6_000_000 + k / 600_000) / 9
        assert abs(m - 1 / rate) <= 0.5 + 1e-6, k
    for bad in ((6, 6, 10, 1, 6), (0, 6, 10, 2, 6), (6, 6, 1, 2, 6)):
        with pytest.raises(ValueError):
            isim.LoadProfile.ramp(*bad)
    r.time(1 << 40)       # a valid profile for the library


def test_des_handler_takes_one_of_mean_and_profile():
    h = _handler()
    p = isim.LoadProfile.constant(1000)
    with pytest.raises(ValueError):
        isim.DesHandler(h)
    with pytest.raises(ValueError):
        isim.DesHandler(h, 1000, p)
    with pytest.raises(ValueError):
        isim.DesHandler(h, mean_interarrival_ns=1000, profile=p)
    d = isim.DesHandler(h, 6_000_000)
    assert d.params.mean_interarrival_ns == 6_000_000 and d.profile is None
    assert isim.DesHandler(h, mean_interarrival_ns=5).params.mean_interarrival_ns == 5
    dp = isim.DesHandler(h, profile=p)
    assert dp.profile is p and dp.info.n_positions == d.info.n_positions
    for name in ("LoadProfile", "profile_arrivals", "profile_arrivals_device", "profile_arrivals_workspace_bytes"):
        assert callable(getattr(isim, name)), name
