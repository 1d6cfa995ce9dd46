"""Closed-loop clients on the CPU: the header's declarations,
isim_closed_loop_schedule and isim_closed_loop_host against the rule in Python
integers, saturation, chaining, every argument the entry points reject (all on
the host, before any HIP call) and the Python builders."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import isim
from isim import native

from conftest import ROOT

HDR = open(os.path.join(ROOT, "include", "isim.h")).read()
U64 = np.uint64
TOP = (1 << 64) - 1
FUNCS = ("isim_closed_loop_schedule", "isim_closed_loop_host", "isim_closed_loop_workspace_bytes",
         "isim_closed_loop_device", "isim_closed_loop")


# ---- the rule in Python integers
def sat(x):
    return min(x, TOP)


def rule(C_, p, uniform, first, lat, F):
    """(arrivals, F after, info) of the batch; F is a list of C Python ints, not modified."""
    F, A, late, sum_late = list(F), [], 0, 0
    for i, L in enumerate(lat):
        j = first + i
        c, k = j % C_, j // C_
        s = (c * p // C_ if uniform else 0) + k * p
        a = max(F[c], s)
        A.append(a)
        F[c] = sat(a + int(L))
        late += a > s
        sum_late += a - s
    return A, F, [max(F), min(F), late, sum_late & TOP]


def records(lat):
    r = np.zeros(len(lat), isim.REC_DTYPE)
    r["latency_ns"] = np.array(lat, dtype=U64)
    return r


def latencies(rng, n):
    lat = rng.integers(0, 1 << 20, n, dtype=np.uint64)
    lat[rng.random(n) < 0.1] = 0
    return lat


# ---- declarations
def test_header_and_bindings():
    assert re.search(r"#define\s+ISIM_CL_MAX_CONNECTIONS\s+65536u", HDR) and native.CL_MAX_CONNECTIONS == 65536
    assert re.search(r"#define\s+ISIM_CL_UNIFORM\s+1u", HDR) and native.CL_UNIFORM == 1
    for name, v in (("MAKESPAN", 0), ("MIN_FREE", 1), ("LATE", 2), ("SUM_LATE", 3), ("INFO_WORDS", 4)):
        assert re.search(r"#define\s+ISIM_CL_%s\s+%d\b" % (name, v), HDR) and getattr(native, "CL_" + name) == v
    assert re.search(r"struct isim_closed_loop \{[^}]*connections;[^}]*flags;[^}]*period_ns;[^}]*first_index;[^}]*\};",
                     HDR)
    assert C.sizeof(native.ClosedLoop) == 24
    lib = native.load()
    for fn in FUNCS:
        assert re.search(r"ISIM_API int %s\(" % fn, HDR), fn
        assert fn in native.SIGNATURES and hasattr(lib, fn), fn
    assert re.search(r"#define\s+ISIM_ABI_VERSION\s+10\b", HDR) and lib.isim_abi_version() == 10


# ---- the host functions against the rule
@pytest.mark.parametrize("uniform", [False, True])
@pytest.mark.parametrize("C_", [1, 2, 3, 5, 64, 1000])
def test_schedule_and_host_against_rule(C_, uniform):
    rng = np.random.default_rng(100 + C_)
    for p in (0, 1, 997, 1 << 40):
        cl = isim.ClosedLoop(C_, period_ns=p, uniform=uniform)
        for j in (0, 1, C_ - 1, C_, C_ + 1, 12345, (1 << 40) - 3, (1 << 40) + 4999):
            want = (j % C_, (j % C_ * p // C_ if uniform else 0) + j // C_ * p)
            if want[1] >= 1 << 63:
                with pytest.raises(isim.IsimError):
                    cl.schedule(j)
            else:
                assert cl.schedule(j) == want, (p, j)
        for first in (0, 7, (1 << 40) - 3):
            for n in (0, 1, C_, 5000):
                if p == 1 << 40 and first + n > (1 << 22) * C_:
                    continue      # past the schedule bound: test_einval
                lat = latencies(rng, n)
                F0 = [int(x) for x in rng.integers(0, 1 << 21, C_)] if n % 2 else [0] * C_
                A, F, info = rule(C_, p, uniform, first, lat, F0)
                a, f, i = cl.arrivals_host(records(lat), first, np.array(F0, U64) if n % 2 else None)
                assert a.tolist() == A and f.tolist() == F and i.tolist() == info, (p, first, n)


def test_schedule_bound_is_exact():
    """p = 2^40: k = 2^23 - 1 is the last request whose start is below 2^63."""
    cl = isim.ClosedLoop(3, period_ns=1 << 40)
    last = ((1 << 23) - 1) * 3 + 2
    assert cl.schedule(last) == (2, ((1 << 23) - 1) << 40)
    with pytest.raises(isim.IsimError) as e:
        cl.schedule(last + 1)
    assert e.value.status == "EINVAL"
    rec = records([5, 5])
    cl.arrivals_host(rec, last - 1)
    with pytest.raises(isim.IsimError):
        cl.arrivals_host(rec, last)


def test_saturation():
    rng = np.random.default_rng(5)
    for C_, p, uniform in ((1, 0, False), (3, 997, True), (64, 1 << 30, False)):
        lat = [int(x) for x in latencies(rng, 2000)]
        for at, v in ((100, 1 << 63), (101, 1 << 63), (500, TOP), (501, 3), (1999, TOP)):
            lat[at] = v
        A, F, info = rule(C_, p, uniform, 11, lat, [0] * C_)
        a, f, i = isim.ClosedLoop(C_, period_ns=p, uniform=uniform).arrivals_host(records(lat), 11)
        assert a.tolist() == A and f.tolist() == F and i.tolist() == info
        assert TOP in F and info[0] == TOP


def test_chaining_and_untouched_connections():
    rng = np.random.default_rng(6)
    for C_, p, uniform in ((5, 0, False), (64, 300_000, True), (1000, 997, False)):
        cl = isim.ClosedLoop(C_, period_ns=p, uniform=uniform)
        n, first = 5000, 7
        rec = records(latencies(rng, n))
        a, f, info = cl.arrivals_host(rec, first)
        cuts, state, parts, late, sum_late = (0, 1234, 1234 + C_ // 2, n), None, [], 0, 0
        for lo, hi in zip(cuts, cuts[1:]):
            pa, state, pi = cl.arrivals_host(rec[lo:hi], first + lo, state)
            parts.append(pa)
            late, sum_late = late + int(pi[native.CL_LATE]), sum_late + int(pi[native.CL_SUM_LATE])
        assert np.array_equal(np.concatenate(parts), a) and np.array_equal(state, f)
        assert pi[:2].tolist() == info[:2].tolist() and [late, sum_late & TOP] == info[2:].tolist()
    # a batch of 3 requests on 1000 connections: the other 997 keep their state
    cl = isim.ClosedLoop(1000)
    F0 = np.arange(1000, dtype=U64) + U64(10)
    _, f, info = cl.arrivals_host(records([1, 2, 3]), 998, F0)
    want = F0.copy()
    want[[998, 999, 0]] = [1008 + 1, 1009 + 2, 10 + 3]
    assert np.array_equal(f, want) and info[:2].tolist() == [1011, 11]
    # n 0: the totals of the incoming state, nothing else
    _, f, info = cl.arrivals_host(records([]), 5, F0)
    assert np.array_equal(f, F0) and info.tolist() == [1009, 10, 0, 0]


# ---- every EINVAL, with no GPU
def _rc(fn, *args):
    rc = fn(*args)
    assert rc in (native.OK, native.EINVAL), (rc, native.last_error())
    return rc


def test_einval():
    lib = native.load()
    raw = np.zeros(4 * 16 + 16, np.uint8)      # the records at a 16-byte boundary, whatever numpy returned
    off = -raw.ctypes.data % 16
    rec = raw[off:off + 64].view(isim.REC_DTYPE)
    rec["latency_ns"] = [1, 2, 3, 4]
    arr, F, info = np.zeros(4, U64), np.zeros(8, U64), np.zeros(4, U64)
    ws = np.zeros(1 << 14, U64)
    R, A, Fp, I, W = rec.ctypes.data, arr.ctypes.data, F.ctypes.data, info.ctypes.data, ws.ctypes.data

    def calls(cl, n=4, r=R, a=A, f=Fp, i=I, w=W, wsb=ws.nbytes, device_only=False):
        """The return codes of the three batch entry points for one set of arguments, which at
        least the device ones must refuse before any HIP call (device_only: the device entry's own
        checks, which the others do not make)."""
        p = C.byref(cl) if cl is not None else None
        dev = _rc(lib.isim_closed_loop_device, p, r, n, f, a, i, w, wsb, None)
        if device_only:
            return dev
        return [_rc(lib.isim_closed_loop_host, p, r, n, f, a, i), dev, _rc(lib.isim_closed_loop, 0, p, r, n, f, a, i)]

    good = native.ClosedLoop(8, 0, 1000, 0)
    assert _rc(lib.isim_closed_loop_host, C.byref(good), R, 4, Fp, A, I) == native.OK
    bad_clients = [None, native.ClosedLoop(0, 0, 0, 0), native.ClosedLoop(65537, 0, 0, 0),
                   native.ClosedLoop(8, 2, 0, 0), native.ClosedLoop(8, 0x80000001, 0, 0),
                   native.ClosedLoop(8, 0, (1 << 40) + 1, 0)]
    for cl in bad_clients:
        assert calls(cl) == [native.EINVAL] * 3, cl and (cl.connections, cl.flags, cl.period_ns)
        c, s = C.c_uint32(), C.c_uint64()
        assert lib.isim_closed_loop_schedule(C.byref(cl) if cl is not None else None, 0, C.byref(c),
                                             C.byref(s)) == native.EINVAL
    assert lib.isim_closed_loop_schedule(C.byref(good), 0, None, C.byref(C.c_uint64())) == native.EINVAL
    assert lib.isim_closed_loop_schedule(C.byref(good), 0, C.byref(C.c_uint32()), None) == native.EINVAL
    # first_index, n, the schedule bound
    assert calls(native.ClosedLoop(8, 0, 1000, (1 << 40) + 1)) == [native.EINVAL] * 3
    assert calls(good, n=(1 << 32) + 1) == [native.EINVAL] * 3
    assert calls(native.ClosedLoop(1, 0, 1 << 40, 1 << 23)) == [native.EINVAL] * 3
    # p = 2^40 - 1, row 2^23: connection 0 starts at 2^63 - 2^23, connection 1 an eighth of a period later
    edge = native.ClosedLoop(8, native.CL_UNIFORM, (1 << 40) - 1, 8 << 23)
    assert calls(edge, n=2) == [native.EINVAL] * 3
    assert _rc(lib.isim_closed_loop_host, C.byref(edge), R, 1, Fp, A, I) == native.OK
    edge.flags = 0
    assert _rc(lib.isim_closed_loop_host, C.byref(edge), R, 4, Fp, A, I) == native.OK
    assert _rc(lib.isim_closed_loop_host, C.byref(native.ClosedLoop(8, 0, 1 << 40, 8 * ((1 << 23) - 1))), R, 4, Fp, A,
               I) == native.OK
    # null pointers
    assert calls(good, r=None) == [native.EINVAL] * 3
    assert calls(good, a=None) == [native.EINVAL] * 3
    assert calls(good, i=None) == [native.EINVAL] * 3
    assert calls(good, w=None, device_only=True) == native.EINVAL
    # alignment (device entry): records 16 bytes, the others 8
    for kw in ({"r": R + 8}, {"a": A + 4}, {"f": Fp + 4}, {"i": I + 4}, {"w": W + 4}):
        assert calls(good, device_only=True, **kw) == native.EINVAL, kw
    # the workspace
    need = isim.closed_loop_workspace_bytes(4, 8)
    assert need > 0 and calls(good, wsb=need - 1, device_only=True) == native.EINVAL
    assert "isim_closed_loop_workspace_bytes" in native.last_error()
    b = C.c_uint64()
    assert lib.isim_closed_loop_workspace_bytes(4, 8, None) == native.EINVAL
    assert lib.isim_closed_loop_workspace_bytes(4, 0, C.byref(b)) == native.EINVAL
    assert lib.isim_closed_loop_workspace_bytes(4, 65537, C.byref(b)) == native.EINVAL
    assert lib.isim_closed_loop_workspace_bytes((1 << 32) + 1, 8, C.byref(b)) == native.EINVAL
    assert lib.isim_closed_loop_workspace_bytes(0, 8, C.byref(b)) == native.OK and b.value == 0


def test_workspace_is_a_sixteenth_of_the_arrivals():
    """One 16-byte map per row block and connection, row blocks of at least 16 rows: at most n + 2 rows' worth."""
    for C_ in (1, 4, 63, 64, 100, 256, 1000, 65536):
        for n in (1, 8192, (1 << 22) + 5, 1 << 32):
            b = isim.closed_loop_workspace_bytes(n, C_)
            assert b % 16 == 0 and 16 * C_ <= b <= n + 16 * C_ * 2, (C_, n, b)


# ---- the Python builders
def test_builders():
    c = isim.ClosedLoop()
    assert (c.connections, c.period_ns, c.uniform) == (64, 0, False)
    assert isim.ClosedLoop(64, qps=1000).period_ns == 64_000_000
    assert isim.ClosedLoop(3, qps=7).period_ns == 3 * 10**9 // 7
    assert isim.ClosedLoop(1, qps=0.5).period_ns == 2 * 10**9
    assert isim.ClosedLoop(4, period_ns=5, uniform=True).c(9).first_index == 9
    for kw in ({"qps": 0}, {"qps": -1}, {"qps": 1e12}, {"qps": 1e-4}, {"qps": 10, "period_ns": 5}):
        with pytest.raises(ValueError):
            isim.ClosedLoop(64, **kw)
    with pytest.raises(ValueError):
        isim.ClosedLoop(4).arrivals_host(records([1]), 0, np.zeros(3, U64))
    with pytest.raises(ValueError):
        isim.ClosedLoopRun(None, c, 10**9, 3 * 10**8)
    assert isim.ClosedLoopRun(None, c, 10**9, 10**8).n_windows == 10
    d = isim.decode_closed_loop_info(np.array([9, 3, 2, 7], U64))
    assert d == {"makespan_ns": 9, "min_free_ns": 3, "late": 2, "sum_late_ns": 7}
