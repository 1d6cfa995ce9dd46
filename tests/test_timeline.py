"""The load-test timeline on the CPU: the header's constants,
the argument checks of isim_des_arrivals* and isim_timeline* (all made on the
host before any HIP call), the host merge, and decode_timeline's derived
series on a hand-made table."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import isim
from isim import native

from conftest import ROOT

HDR = open(os.path.join(ROOT, "include", "isim.h")).read()
U64 = np.uint64
W = native.TL_ROW_WORDS


def _define(name):
    m = re.search(r"#define\s+%s\s+\(?\s*([0-9]+)u?\b" % name, HDR)
    assert m, name
    return int(m.group(1))


def test_header_constants():
    assert _define("ISIM_TL_MAX_WINDOWS") == native.TL_MAX_WINDOWS == 65536
    for name, v in (("ARRIVED", native.TL_ARRIVED), ("DONE", native.TL_DONE), ("SUM_LAT", native.TL_SUM_LAT),
                    ("MAX_LAT", native.TL_MAX_LAT), ("PROM", native.TL_PROM)):
        assert _define("ISIM_TL_" + name) == v, name
    assert re.search(r"#define\s+ISIM_TL_ROW_WORDS\s+\(7 \+ 2 \* ISIM_N_PROM\)", HDR)
    assert native.TL_ROW_WORDS == 7 + 2 * native.N_PROM == 73
    assert C.sizeof(native.TimelineParams) == 24


def test_out_words():
    assert isim.timeline_out_words(1) == 3 * 73
    assert isim.timeline_out_words(65536) == 65538 * 73


def test_arrivals_workspace_bytes():
    prev = 0
    for n in (1, 2, 8191, 8192, 8193, 70_001, 1 << 20, 8192 * 1024 + 8193, 1 << 31, 1 << 40):
        b = isim.des_arrivals_workspace_bytes(n)
        assert b > 0 and b >= prev and b >= 8 * ((n + 8191) // 8192 + 1), n
        prev = b
    with pytest.raises(isim.IsimError) as e:
        isim.des_arrivals_workspace_bytes((1 << 40) + 1)
    assert e.value.status == "EINVAL"
    assert native.load().isim_des_arrivals_workspace_bytes(1, None) == native.EINVAL


def _handler():
    doc = {"services": [{"name": "a", "isEntrypoint": True, "script": [{"sleep": "1ms"}]}]}
    return isim.Handler(isim.ServiceGraph.from_json(json.dumps(doc)), None, isim.SimParams())


def test_arrivals_einval():
    """Every rejected argument, before any HIP call (no GPU here).  The
    pointers are fake device addresses: a call that got past the checks would
    fail with another status."""
    lib, h = native.load(), _handler()
    ok = native.DesParams(1000, 0, 0)
    buf, ws, wsb = 0x10000, 0x20000, isim.des_arrivals_workspace_bytes(100)

    def dev(hh=h._h, p=ok, n=100, a=buf, w=ws, b=wsb):
        return lib.isim_des_arrivals_device(hh, C.byref(p) if p is not None else None, 0, n, a, w, b, None)

    def host(hh=h._h, p=ok, n=100, a=buf):
        return lib.isim_des_arrivals(hh, 0, C.byref(p) if p is not None else None, 0, n, a)

    for f in (dev, host):
        assert f(hh=None) == native.EINVAL
        assert f(p=None) == native.EINVAL
        assert f(a=None) == native.EINVAL
        assert f(p=native.DesParams(0, 0, 0)) == native.EINVAL
        assert f(p=native.DesParams((1 << 34) + 1, 0, 0)) == native.EINVAL
        assert f(p=native.DesParams(1000, 0, 1)) == native.EINVAL
        assert f(p=native.DesParams(1000, 2, 0)) == native.EINVAL
        assert f(p=native.DesParams(1000, 3, 0)) == native.EINVAL
        # nothing to do: OK without touching anything, WIDE accepted, null buffer fine
        assert f(n=0, a=None) == native.OK
        assert f(n=0, a=None, p=native.DesParams(1 << 34, native.DES_FLAG_WIDE, 0)) == native.OK
    assert dev(w=None) == native.EINVAL
    assert dev(b=wsb - 1) == native.EINVAL
    assert dev(b=0) == native.EINVAL
    assert dev(n=8193, b=isim.des_arrivals_workspace_bytes(8193) - 256) == native.EINVAL
    assert "workspace" in native.last_error()


def test_timeline_einval():
    lib = native.load()
    ok = native.TimelineParams(0, 1000, 4, 0)
    arr, rec, out = 0x10000, 0x20000, 0x30000

    def dev(a=arr, r=rec, n=10, p=ok, o=out):
        return lib.isim_timeline_device(a, r, n, C.byref(p) if p is not None else None, o, None)

    def host(a=arr, r=rec, n=10, p=ok, o=out):
        return lib.isim_timeline(0, a, r, n, C.byref(p) if p is not None else None, o)

    for f in (dev, host):
        assert f(p=None) == native.EINVAL
        assert f(o=None) == native.EINVAL
        assert f(a=None) == native.EINVAL
        assert f(r=None) == native.EINVAL
        assert f(p=native.TimelineParams(0, 0, 4, 0)) == native.EINVAL
        assert f(p=native.TimelineParams(0, 1000, 0, 0)) == native.EINVAL
        assert f(p=native.TimelineParams(0, 1000, 65537, 0)) == native.EINVAL
        assert f(p=native.TimelineParams(0, 1000, 4, 1)) == native.EINVAL
        assert f(n=(1 << 40) + 1) == native.EINVAL
        assert f(n=0, a=None, r=None) == native.OK
        assert f(n=0, a=None, r=None, p=native.TimelineParams((1 << 64) - 1, (1 << 64) - 1, 65536, 0)) == native.OK
    assert dev(r=rec + 8) == native.EINVAL
    assert dev(a=arr + 4) == native.EINVAL
    assert "aligned" in native.last_error()


def _merge_np(a, b, n_windows):
    a, b = a.reshape(n_windows + 2, W), b.reshape(n_windows + 2, W)
    out = a + b
    mx = slice(native.TL_MAX_LAT, native.TL_MAX_LAT + 2)
    out[:, mx] = np.maximum(a[:, mx], b[:, mx])
    return out.reshape(-1)


@pytest.mark.parametrize("n_windows", [1, 7, 4096])
def test_merge_against_numpy(n_windows):
    rng = np.random.default_rng(n_windows)
    words = isim.timeline_out_words(n_windows)
    a = rng.integers(0, 1 << 62, words, dtype=np.uint64)
    b = rng.integers(0, 1 << 62, words, dtype=np.uint64)
    # maxima over the whole u64 range, either side the larger
    for t in (a, b):
        t.reshape(-1, W)[:, native.TL_MAX_LAT:native.TL_MAX_LAT + 2] = rng.integers(
            0, 1 << 64, (n_windows + 2, 2), dtype=np.uint64)
    want = _merge_np(a.copy(), b, n_windows)
    got = isim.timeline_merge(n_windows, a.copy(), b)
    assert np.array_equal(got, want)
    mx = got.reshape(-1, W)[:, native.TL_MAX_LAT]
    assert (mx >= a.reshape(-1, W)[:, native.TL_MAX_LAT]).all() and (mx >= b.reshape(-1, W)[:, native.TL_MAX_LAT]).all()
    lib = native.load()
    assert lib.isim_timeline_merge(0, a.ctypes.data, b.ctypes.data) == native.EINVAL
    assert lib.isim_timeline_merge(65537, a.ctypes.data, b.ctypes.data) == native.EINVAL
    assert lib.isim_timeline_merge(n_windows, None, b.ctypes.data) == native.EINVAL
    assert lib.isim_timeline_merge(n_windows, a.ctypes.data, None) == native.EINVAL


def test_decode_hand_made_table():
    """3 windows of 1 s from t0 = 5 s.  10 requests: 2 arrive before t0 (one of
    them also completes there), 3 + 4 + 0 in the windows, 1 after the last."""
    n_windows, t0, win = 3, 5_000_000_000, 1_000_000_000
    t = np.zeros((n_windows + 2, W), U64)
    A, D, S, M, P = native.TL_ARRIVED, native.TL_DONE, native.TL_SUM_LAT, native.TL_MAX_LAT, native.TL_PROM
    t[:, A] = [2, 3, 4, 0, 1]
    t[:, D] = [1, 2, 1, 3, 1]          # 200s
    t[:, D + 1] = [0, 0, 2, 0, 0]      # 500s
    t[:, S] = [10, 30, 5, 600, 7]
    t[:, S + 1] = [0, 0, 44, 0, 0]
    t[:, M] = [10, 20, 5, 300, 7]
    t[:, M + 1] = [0, 0, 40, 0, 0]
    t[:, P + 0] = t[:, D]              # all in the first bucket
    t[2, P + native.N_PROM + 32] = 2   # the 500s of window 1 in +Inf
    d = isim.decode_timeline(t.reshape(-1), n_windows, t0, win)
    assert list(d["t_start_ns"]) == [5_000_000_000, 6_000_000_000, 7_000_000_000]
    assert d["arrived"].tolist() == [3, 4, 0]
    assert d["done"].tolist() == [[2, 1, 3], [0, 2, 0]]
    assert d["sum_latency_ns"].tolist() == [[30, 5, 600], [0, 44, 0]]
    assert d["max_latency_ns"].tolist() == [[20, 5, 300], [0, 40, 0]]
    assert d["prom"].shape == (2, 3, native.N_PROM)
    assert d["prom"][0, :, 0].tolist() == [2, 1, 3] and int(d["prom"][1, 1, 32]) == 2
    assert int(d["prom"].sum()) == 8
    # the outer rows are kept apart
    assert int(d["before"]["arrived"]) == 2 and d["before"]["done"].tolist() == [1, 0]
    assert int(d["after"]["arrived"]) == 1 and d["after"]["done"].tolist() == [1, 0]
    assert int(d["after"]["sum_latency_ns"][0]) == 7 and d["before"]["prom"].shape == (2, native.N_PROM)
    # in flight at the end of window w: arrivals minus completions up to it, "before" included
    arrived = np.cumsum([2, 3, 4, 0])
    done = np.cumsum([1, 2, 3, 3])
    assert d["in_flight_end"].tolist() == (arrived - done)[1:].tolist() == [2, 3, 0]
    assert d["in_flight_end"].dtype == np.uint64
    # every request is accounted for: in flight after the last window + what arrives later = completions after it
    assert int(d["in_flight_end"][-1]) + int(d["after"]["arrived"]) == int(d["after"]["done"].sum())
    assert d["throughput_per_s"].tolist() == [2.0, 3.0, 3.0]
    m = d["mean_latency_ns"]
    assert m[0].tolist() == [15.0, 5.0, 200.0] and m[1, 1] == 22.0 and np.isnan(m[1, 0])
    # a window in ms: the ratio is per second
    assert isim.decode_timeline(t.reshape(-1), n_windows, 0, 1_000_000)["throughput_per_s"].tolist() == [2e3, 3e3, 3e3]
    # t_start_ns does not wrap
    big = isim.decode_timeline(np.zeros(3 * W, U64), 1, (1 << 64) - 1, (1 << 64) - 1)
    assert list(big["t_start_ns"]) == [(1 << 64) - 1]


def test_python_surface():
    for name in ("des_arrivals", "des_arrivals_device", "timeline", "timeline_device", "timeline_out_words",
                 "decode_timeline"):
        assert callable(getattr(isim, name)), name
    assert callable(isim.DesHandler.arrivals) and callable(isim.DesHandler.timeline)


def test_go_symbols():
    src = open(os.path.join(ROOT, "go", "isim", "isim.go")).read()
    for fn in ("isim_des_arrivals", "isim_timeline"):
        assert "C." + fn + "(" in src, fn
        assert re.search(r"\b%s\b" % fn, HDR)
    assert re.search(r"^func \(h \*Handler\) DesArrivals\(", src, re.M)
    assert re.search(r"^func Timeline\(", src, re.M)
    assert "C.isim_timeline_params" in src and "C.ISIM_TL_ROW_WORDS" in src
