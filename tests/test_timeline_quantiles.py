"""Per-window exact latency percentiles on the CPU: the
header's constants, the workspace size, every argument isim_timeline_quantiles*
rejects (all checks are made on the host before any HIP call), the ppm rule
and timeline_quantiles' decoding on a hand-made table.  No GPU call."""
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
MAX_N = (1 << 32) - 1


def test_header_constants():
    m = re.search(r"#define\s+ISIM_TLQ_OUT_WORDS\(n_windows, n_q\)\s+(.*)", HDR)
    assert m and m.group(1).strip() == "(((uint64_t)(n_windows) + 2) * ISIM_Q_OUT_WORDS(n_q))"
    assert re.search(r"#define\s+ISIM_Q_OUT_WORDS\(n_q\)\s+\(3 \* \(1 \+ \(uint64_t\)\(n_q\)\)\)", HDR)
    assert re.search(r"#define\s+ISIM_ABI_VERSION\s+10\b", HDR) and native.ABI_VERSION == 10
    assert native.MAX_QUANTILES == 16 and (native.Q_ALL, native.Q_200, native.Q_500) == (0, 1, 2)
    for fn in ("isim_timeline_quantiles_workspace_bytes", "isim_timeline_quantiles_device", "isim_timeline_quantiles"):
        assert re.search(r"ISIM_API int %s\(" % fn, HDR) and fn in native.SIGNATURES, fn
    assert "2^32 - 1" in HDR[HDR.index("per-window exact latency percentiles"):]   # the limit on n is stated


def test_out_words():
    assert isim.timeline_quantiles_out_words(1, 1) == 3 * 3 * 2
    assert isim.timeline_quantiles_out_words(60, 5) == 62 * 3 * 6 == 62 * isim.quantiles_out_words(5)
    assert isim.timeline_quantiles_out_words(65536, 16) == 65538 * 51


def test_workspace_bytes():
    f = isim.timeline_quantiles_workspace_bytes
    for n_windows in (1, 2, 37, 4096, 65536):
        prev = 0
        for n in (0, 1, 63, 64, 65, 1000, 70_001, 1 << 20, 1 << 24, 1 << 31, MAX_N):
            b = f(n, n_windows, 5)
            assert b >= 8 * n and b >= prev and b > 0, (n, n_windows)
            prev = b
    for n in (0, 1000, MAX_N):
        prev = 0
        for n_windows in (1, 2, 3, 37, 4096, 65535, 65536):
            b = f(n, n_windows, 16)
            # the 32-bit counters: at least one word per (row, code)
            assert b >= prev and b >= 8 * n + 4 * 2 * (n_windows + 2), (n, n_windows)
            prev = b
    lib = native.load()
    b = C.c_uint64()
    assert lib.isim_timeline_quantiles_workspace_bytes(10, 4, 5, None) == native.EINVAL
    for bad in ((MAX_N + 1, 4, 5), (10, 0, 5), (10, 65537, 5), (10, 4, 0), (10, 4, 17)):
        assert lib.isim_timeline_quantiles_workspace_bytes(*bad, C.byref(b)) == native.EINVAL, bad


def _ppm(*v):
    return (C.c_uint32 * len(v))(*v)


def test_einval():
    """Every rejected argument, before any HIP call (no GPU here).  The
    pointers are fake device addresses: a call that got past the checks would
    fail with another status."""
    lib = native.load()
    ok = native.TimelineParams(0, 1000, 4, 0)
    arr, rec, out, ws = 0x10000, 0x20000, 0x30000, 0x40000
    q5 = _ppm(500000, 750000, 900000, 990000, 999000)
    wsb = isim.timeline_quantiles_workspace_bytes(10, 4, 5)

    def dev(a=arr, r=rec, n=10, p=ok, q=q5, nq=5, o=out, w=ws, b=wsb):
        return lib.isim_timeline_quantiles_device(a, r, n, C.byref(p) if p is not None else None, q, nq, o, w, b, None)

    def host(a=arr, r=rec, n=10, p=ok, q=q5, nq=5, o=out):
        return lib.isim_timeline_quantiles(0, a, r, n, C.byref(p) if p is not None else None, q, nq, o)

    for f in (dev, host):
        # the §14 parameter errors
        assert f(p=None) == native.EINVAL
        assert f(p=native.TimelineParams(0, 0, 4, 0)) == native.EINVAL
        assert f(p=native.TimelineParams(0, 1000, 0, 0)) == native.EINVAL
        assert f(p=native.TimelineParams(0, 1000, 65537, 0)) == native.EINVAL
        assert f(p=native.TimelineParams(0, 1000, 4, 1)) == native.EINVAL
        # the §13 quantile-list errors
        assert f(nq=0) == native.EINVAL
        assert f(nq=17, q=_ppm(*([1] * 17))) == native.EINVAL
        assert f(q=None) == native.EINVAL
        assert f(q=_ppm(500000, 1000001, 0, 0, 0)) == native.EINVAL
        assert "q_ppm[1]" in native.last_error()
        # n and the pointers
        assert f(n=MAX_N + 1) == native.EINVAL
        assert "2^32" in native.last_error()
        assert f(n=1 << 40) == native.EINVAL
        assert f(o=None) == native.EINVAL
        assert f(a=None) == native.EINVAL
        assert f(r=None) == native.EINVAL
    assert dev(w=None) == native.EINVAL
    assert dev(r=rec + 8) == native.EINVAL
    assert "aligned" in native.last_error()
    assert dev(a=arr + 4) == native.EINVAL
    assert dev(o=out + 4) == native.EINVAL
    assert dev(w=ws + 4) == native.EINVAL
    assert dev(b=wsb - 1) == native.EINVAL
    assert "workspace" in native.last_error()
    assert dev(b=0) == native.EINVAL
    # an empty batch still needs its output, its workspace and a valid list
    assert dev(n=0, a=None, r=None, o=None) == native.EINVAL
    assert dev(n=0, a=None, r=None, w=None) == native.EINVAL
    assert dev(n=0, a=None, r=None, nq=0) == native.EINVAL
    assert dev(n=0, a=None, r=None, b=isim.timeline_quantiles_workspace_bytes(0, 4, 5) - 1) == native.EINVAL
    assert host(n=0, a=None, r=None, o=None) == native.EINVAL
    # the workspace grows with n and with the windows
    assert dev(n=11) == native.EINVAL
    assert dev(p=native.TimelineParams(0, 1000, 4096, 0)) == native.EINVAL
    assert "workspace" in native.last_error()


def test_python_rejects_before_the_library():
    with pytest.raises(ValueError):
        isim.timeline_quantiles(np.zeros(3, U64), np.zeros(2, isim.REC_DTYPE), 1000, 4)
    for bad in (0.9999999, 0.1234567, 1.0000001, -0.000001, 1.5):
        with pytest.raises(ValueError):
            isim.timeline_quantiles(np.zeros(2, U64), np.zeros(2, isim.REC_DTYPE), 1000, 4, q=(0.5, bad))
        with pytest.raises(ValueError):
            isim.timeline_quantiles_device(0x10000, 0x20000, 2, 1000, 4, q=(bad,), d_out=0x30000, d_workspace=0x40000)
    # the library's errors come through as IsimError
    with pytest.raises(isim.IsimError) as e:
        isim.timeline_quantiles_device(0x10000, 0x20000, 2, 0, 4, d_out=0x30000, d_workspace=0x40000)
    assert e.value.status == "EINVAL" and "window_ns" in str(e.value)
    with pytest.raises(isim.IsimError) as e:
        isim.timeline_quantiles_device(0x10000, 0x20000, 2, 1000, 4, q=(), d_out=0x30000, d_workspace=0x40000)
    assert e.value.status == "EINVAL"


def test_decode_hand_made_table():
    """2 windows of 1 s from t0 = 5 s, q = (0.5, 1.0): rows before, w0, w1, after."""
    n_windows, t0, win, q = 2, 5_000_000_000, 1_000_000_000, (0.5, 1.0)
    t = np.zeros((n_windows + 2, 3, 3), U64)
    t[0] = [[1, 7, 7], [1, 7, 7], [0, 0, 0]]
    t[1] = [[5, 30, 90], [3, 20, 40], [2, 80, 90]]
    t[2] = [[0, 0, 0], [0, 0, 0], [0, 0, 0]]
    t[3] = [[2, 11, (1 << 64) - 1], [0, 0, 0], [2, 11, (1 << 64) - 1]]
    d = isim.decode_timeline_quantiles(t.reshape(-1), n_windows, t0, win, len(q))
    assert list(d["t_start_ns"]) == [5_000_000_000, 6_000_000_000]
    assert d["count"].shape == (3, 2) and d["count"].tolist() == [[5, 0], [3, 0], [2, 0]]
    assert d["latency_ns"].shape == (3, 2, 2) and d["latency_ns"].dtype == np.uint64
    assert d["latency_ns"][native.Q_ALL].tolist() == [[30, 0], [90, 0]]
    assert d["latency_ns"][native.Q_200].tolist() == [[20, 0], [40, 0]]
    assert d["latency_ns"][native.Q_500].tolist() == [[80, 0], [90, 0]]
    assert d["before"]["count"].tolist() == [1, 1, 0] and d["before"]["latency_ns"].tolist() == [[7, 7], [7, 7], [0, 0]]
    assert d["after"]["count"].tolist() == [2, 0, 2]
    assert d["after"]["latency_ns"].tolist() == [[11, (1 << 64) - 1], [0, 0], [11, (1 << 64) - 1]]
    big = isim.decode_timeline_quantiles(np.zeros(3 * 3 * 2, U64), 1, (1 << 64) - 1, (1 << 64) - 1, 1)
    assert list(big["t_start_ns"]) == [(1 << 64) - 1]


def test_python_surface():
    for name in ("timeline_quantiles", "timeline_quantiles_table", "timeline_quantiles_device",
                 "timeline_quantiles_workspace_bytes", "timeline_quantiles_out_words", "decode_timeline_quantiles"):
        assert callable(getattr(isim, name)), name
    assert callable(isim.DesHandler.timeline_quantiles)


def test_go_symbols():
    src = open(os.path.join(ROOT, "go", "isim", "isim.go")).read()
    assert "C.isim_timeline_quantiles(" in src
    assert re.search(r"^func TimelineQuantiles\(", src, re.M)
