"""The mergeable latency sketch on the CPU: the header's
macros, the bucket rule against a restatement in Python integers, the host
merge and quantile brackets on hand-made tables, and every argument the entry
points reject (all checks are made on the host before any HIP call).  No GPU
call."""
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
MAXU = (1 << 64) - 1
SUB_BITS = range(8)


# ---- the rule restated: Python integers, no shared code with the library
def py_bins(s):
    return (65 - s) * 2**s


def py_bucket(s, v):
    if v < 2 ** (s + 1):
        return v
    shift = v.bit_length() - (s + 1)
    return shift * 2**s + v // 2**shift


def py_bounds(s, b):
    if b < 2 ** (s + 1):
        return b, b
    shift = b // 2**s - 1
    lo = (2**s + b % 2**s) * 2**shift
    return lo, lo + 2**shift - 1


def rule_values(s, seed=0):
    vals = {0, 1, 2 ** (s + 1) - 1, 2 ** (s + 1), MAXU}
    for k in range(64):
        vals.update((2**k - 1, 2**k, 2**k + 1))
    rng = np.random.default_rng(seed + s)
    vals.update(int(x) for x in rng.integers(0, 1 << 64, 300, dtype=np.uint64))
    vals.update(int(x) >> int(sh) for x, sh in zip(rng.integers(0, 1 << 64, 300, dtype=np.uint64),
                                                   rng.integers(0, 64, 300)))
    return sorted(vals)


def test_header_macros_agree_with_native():
    assert re.search(r"#define\s+ISIM_SK_MAX_SUB_BITS\s+7\b", HDR) and native.SK_MAX_SUB_BITS == 7
    assert re.search(r"#define\s+ISIM_SK_BINS\(s\)\s+\(\(uint64_t\)\(65 - \(s\)\) << \(s\)\)", HDR)
    assert re.search(r"#define\s+ISIM_SK_WORDS\(s\)\s+\(2 \* ISIM_SK_BINS\(s\)\)", HDR)
    assert re.search(r"#define\s+ISIM_TLS_OUT_WORDS\(n_windows, s\)\s+\(\(\(uint64_t\)\(n_windows\) \+ 2\) \* "
                     r"ISIM_SK_WORDS\(s\)\)", HDR)
    assert re.search(r"#define\s+ISIM_SKQ_OUT_WORDS\(n_q\)\s+\(3 \* \(1 \+ 2 \* \(uint64_t\)\(n_q\)\)\)", HDR)
    assert [native.SKQ_OUT_WORDS(n) for n in (1, 5, 16)] == [9, 33, 99]
    assert re.search(r"#define\s+ISIM_ABI_VERSION\s+10\b", HDR) and native.ABI_VERSION == 10
    assert [native.SK_BINS(s) for s in (0, 3, 7)] == [65, 496, 7424]
    for s in SUB_BITS:
        assert native.SK_BINS(s) == py_bins(s) == isim.sketch_bins(s) and isim.sketch_words(s) == 2 * py_bins(s)
        assert native.SK_WORDS(s) == isim.sketch_words(s)
    assert isim.timeline_sketch_out_words(65536, 7) == 65538 * 2 * 7424 < 1 << 32
    assert isim.timeline_sketch_out_words(60, 3) == 62 * 992
    for fn in ("isim_sketch_bucket", "isim_sketch_bounds", "isim_sketch_merge", "isim_sketch_quantiles",
               "isim_latency_sketch_device", "isim_latency_sketch", "isim_timeline_sketch_device",
               "isim_timeline_sketch"):
        assert re.search(r"ISIM_API int %s\(" % fn, HDR) and fn in native.SIGNATURES, fn
    for bad in (-1, 8):
        with pytest.raises(ValueError):
            isim.sketch_bins(bad)


@pytest.mark.parametrize("s", SUB_BITS)
def test_bucket_and_bounds_against_the_restatement(s):
    for v in rule_values(s):
        b = isim.sketch_bucket(s, v)
        assert b == py_bucket(s, v), (s, v)
        lo, hi = isim.sketch_bounds(s, b)
        assert (lo, hi) == py_bounds(s, b) and lo <= v <= hi, (s, v)
    assert isim.sketch_bucket(s, MAXU) == py_bins(s) - 1
    assert isim.sketch_bucket(s, 2 ** (s + 1) - 1) + 1 == isim.sketch_bucket(s, 2 ** (s + 1)) == 2 ** (s + 1)
    if s == 0:   # the bit-length histogram
        assert all(isim.sketch_bucket(0, v) == v.bit_length() for v in rule_values(0))


@pytest.mark.parametrize("s", SUB_BITS)
def test_bins_partition_the_u64_range(s):
    prev_hi = -1
    for b in range(py_bins(s)):
        lo, hi = isim.sketch_bounds(s, b)
        assert lo == prev_hi + 1 and lo <= hi, (s, b)
        assert hi - lo < max(1, lo >> s), (s, b)
        assert (lo, hi) == py_bounds(s, b)
        prev_hi = hi
    assert prev_hi == MAXU
    # both ends of every bin go back to it (every bin at s <= 3, a sample above)
    step = 1 if s <= 3 else 37
    for b in list(range(0, py_bins(s), step)) + [py_bins(s) - 1]:
        lo, hi = isim.sketch_bounds(s, b)
        assert isim.sketch_bucket(s, lo) == b == isim.sketch_bucket(s, hi)
    if s == 7:
        assert all(isim.sketch_bounds(7, v) == (v, v) for v in range(256))   # exact below 256 ns
        lo, hi = isim.sketch_bounds(7, 256)
        assert (lo, hi) == (256, 257)


def _table(s, entries):
    """entries: (code, value, count) -> the table u64[2][bins] with count records at value's bin."""
    t = np.zeros((2, py_bins(s)), U64)
    for code, v, c in entries:
        t[code, py_bucket(s, v)] += U64(c)
    return t.reshape(-1)


def test_merge_against_numpy():
    rng = np.random.default_rng(3)
    for s, rows in ((0, 1), (3, 1), (7, 1), (3, 62), (7, 5)):
        a = rng.integers(0, 1 << 63, rows * 2 * py_bins(s), dtype=np.uint64)
        b = rng.integers(0, 1 << 63, a.size, dtype=np.uint64)
        want = a + b
        got = isim.sketch_merge(s, a, b)
        assert got is a and np.array_equal(a, want)
    a = np.full(2 * 65, MAXU, U64)   # plain u64 addition: it wraps like the device's
    isim.sketch_merge(0, a, np.ones(130, U64))
    assert not a.any()
    with pytest.raises(ValueError):
        isim.sketch_merge(3, np.zeros(991, U64), np.zeros(991, U64))
    with pytest.raises(ValueError):
        isim.sketch_merge(3, np.zeros(992, U64), np.zeros(2 * 992, U64))
    with pytest.raises(ValueError):
        isim.sketch_merge(3, np.zeros(992, np.int64), np.zeros(992, U64))
    with pytest.raises(ValueError):
        isim.sketch_merge(3, np.zeros(0, U64), np.zeros(0, U64))
    with pytest.raises(ValueError):   # dst is written in place: a list is no table
        isim.sketch_merge(3, [0] * 992, np.zeros(992, U64))


def test_quantiles_empty_class_and_one_record():
    for s in (0, 3, 7):
        r = isim.sketch_quantiles(s, np.zeros(2 * py_bins(s), U64))
        assert all(r[c] == {"count": 0, "q": {f: (0, 0) for f in isim.DEFAULT_Q}} for c in ("all", "200", "500"))
        v = 123_456_789
        r = isim.sketch_quantiles(s, _table(s, [(1, v, 1)]), (0.0, 0.5, 1.0))
        want = py_bounds(s, py_bucket(s, v))
        assert r["200"] == {"count": 0, "q": {0.0: (0, 0), 0.5: (0, 0), 1.0: (0, 0)}}
        assert r["500"] == r["all"] == {"count": 1, "q": {0.0: want, 0.5: want, 1.0: want}}
        assert want[0] <= v <= want[1]


def test_quantiles_rank_boundary_straddles_two_bins():
    """500 records in A's bin and 500 in B's: 500,000 ppm is the 500th (A), 500,001 ppm the 501st (B);
    the same by classes when the A's are 200s and the B's 500s."""
    for s in (0, 3, 7):
        a, b = 3_000_000, 900_000_000
        ba, bb = py_bounds(s, py_bucket(s, a)), py_bounds(s, py_bucket(s, b))
        assert ba != bb
        r = isim.sketch_quantiles(s, _table(s, [(0, a, 500), (0, b, 500)]), (0.5, 0.500001, 0.0, 1.0))
        assert r["200"] == r["all"] == {"count": 1000, "q": {0.5: ba, 0.500001: bb, 0.0: ba, 1.0: bb}}
        r = isim.sketch_quantiles(s, _table(s, [(0, a, 500), (1, b, 500)]), (0.5, 0.500001, 1.0))
        assert r["all"]["q"] == {0.5: ba, 0.500001: bb, 1.0: bb}
        assert r["200"] == {"count": 500, "q": {0.5: ba, 0.500001: ba, 1.0: ba}}
        assert r["500"] == {"count": 500, "q": {0.5: bb, 0.500001: bb, 1.0: bb}}


def test_quantiles_sixteen_unsorted_repeated():
    q = (0.999, 0.5, 0.0, 1.0, 0.5, 0.25, 0.999999, 0.000001, 0.9, 0.99, 0.75, 0.9, 0.1, 1.0, 0.333333, 0.5)
    assert len(q) == native.MAX_QUANTILES
    rng = np.random.default_rng(16)
    lat = rng.integers(0, 1 << 40, 5000, dtype=np.uint64) >> rng.integers(0, 30, 5000, dtype=np.uint64)
    code = rng.integers(0, 2, 5000)
    for s in (3, 7):
        t = _table(s, [(int(c), int(v), 1) for c, v in zip(code, lat)])
        r = isim.sketch_quantiles(s, t, q)
        for name, mask in (("all", np.ones(5000, bool)), ("200", code == 0), ("500", code == 1)):
            v = np.sort(lat[mask])
            assert r[name]["count"] == len(v)
            for f in q:
                exact = int(v[max(1, -(-round(f * 1e6) * len(v) // 10**6)) - 1])
                lo, hi = r[name]["q"][f]
                assert lo <= exact <= hi and (lo, hi) == py_bounds(s, py_bucket(s, exact)), (s, name, f)


def _ppm(*v):
    return (C.c_uint32 * len(v))(*v)


def test_quantiles_class_count_limit():
    """A class count of 2^40 is accepted, 2^40 + 1 is EINVAL (isim_quantile_rank's limit), per class and for ALL."""
    lib = native.load()
    s, q, out = 3, _ppm(500000, 1000000), np.zeros(3 * 5, U64)

    def run(t):
        return lib.isim_sketch_quantiles(s, t.ctypes.data, q, 2, out.ctypes.data)

    t = _table(s, [(0, 1000, 1 << 40)])
    assert run(t) == native.OK and int(out[0]) == 1 << 40 == int(out[5]) and int(out[10]) == 0
    t = _table(s, [(0, 1000, 1 << 39), (1, 5000, 1 << 39)])
    assert run(t) == native.OK and int(out[0]) == 1 << 40
    assert (int(out[1]), int(out[2])) == py_bounds(s, py_bucket(s, 1000))       # rank 2^39: the last 200
    assert (int(out[3]), int(out[4])) == py_bounds(s, py_bucket(s, 5000))
    for bad in ([(0, 1000, (1 << 40) + 1)], [(1, 1000, (1 << 40) + 1)], [(0, 1000, 1 << 40), (1, 7, 1)],
                [(0, 1000, 1 << 39), (0, 5000, (1 << 39) + 1)], [(0, 1, MAXU), (0, 2, 2)]):
        assert run(_table(s, bad)) == native.EINVAL, bad
        assert "2^40" in native.last_error()


def test_einval_host_functions():
    lib = native.load()
    b, lo, hi = C.c_uint32(), C.c_uint64(), C.c_uint64()
    assert lib.isim_sketch_bucket(8, 5, C.byref(b)) == native.EINVAL
    assert "sub_bits" in native.last_error()
    assert lib.isim_sketch_bucket(7, 5, None) == native.EINVAL
    assert lib.isim_sketch_bounds(8, 0, C.byref(lo), C.byref(hi)) == native.EINVAL
    assert lib.isim_sketch_bounds(7, 0, None, C.byref(hi)) == native.EINVAL
    assert lib.isim_sketch_bounds(7, 0, C.byref(lo), None) == native.EINVAL
    for s in SUB_BITS:
        assert lib.isim_sketch_bounds(s, py_bins(s), C.byref(lo), C.byref(hi)) == native.EINVAL
        assert lib.isim_sketch_bounds(s, py_bins(s) - 1, C.byref(lo), C.byref(hi)) == native.OK and hi.value == MAXU
    t = np.zeros(2 * py_bins(3), U64)
    assert lib.isim_sketch_merge(8, 1, t.ctypes.data, t.ctypes.data) == native.EINVAL
    assert lib.isim_sketch_merge(3, 1, None, t.ctypes.data) == native.EINVAL
    assert lib.isim_sketch_merge(3, 1, t.ctypes.data, None) == native.EINVAL
    assert lib.isim_sketch_merge(3, 0, t.ctypes.data, t.ctypes.data) == native.EINVAL
    assert lib.isim_sketch_merge(3, 65539, t.ctypes.data, t.ctypes.data) == native.EINVAL
    out = np.zeros(3 * 33, U64)
    q5 = _ppm(500000, 750000, 900000, 990000, 999000)

    def quant(s=3, tab=t.ctypes.data, q=q5, nq=5, o=out.ctypes.data):
        return lib.isim_sketch_quantiles(s, tab, q, nq, o)

    assert quant() == native.OK
    assert quant(s=8) == native.EINVAL
    assert quant(tab=None) == native.EINVAL
    assert quant(o=None) == native.EINVAL
    assert quant(q=None) == native.EINVAL
    assert quant(nq=0) == native.EINVAL
    assert quant(nq=17, q=_ppm(*([1] * 17))) == native.EINVAL
    assert quant(q=_ppm(500000, 1000001, 0, 0, 0)) == native.EINVAL
    assert "q_ppm[1]" in native.last_error()


def test_einval_device_and_synchronous_entries():
    """Every rejected argument of the four GPU entry points, before any HIP call (no GPU
    here).  The pointers are fake device addresses: a call that got past the checks would
    fail with another status."""
    lib = native.load()
    ok = native.TimelineParams(0, 1000, 4, 0)
    arr, rec, tab = 0x10000, 0x20000, 0x30000
    big = (1 << 40) + 1

    def bdev(r=rec, n=10, s=7, t=tab):
        return lib.isim_latency_sketch_device(r, n, s, t, None)

    def bhost(r=rec, n=10, s=7, t=tab):
        return lib.isim_latency_sketch(0, r, n, s, t)

    def wdev(a=arr, r=rec, n=10, p=ok, s=7, o=tab):
        return lib.isim_timeline_sketch_device(a, r, n, C.byref(p) if p is not None else None, s, o, None)

    def whost(a=arr, r=rec, n=10, p=ok, s=7, o=tab):
        return lib.isim_timeline_sketch(0, a, r, n, C.byref(p) if p is not None else None, s, o)

    for f in (bdev, bhost):
        assert f(s=8) == native.EINVAL
        assert "sub_bits" in native.last_error()
        assert f(t=None) == native.EINVAL
        assert f(r=None) == native.EINVAL
        assert f(n=big) == native.EINVAL
        assert "2^40" in native.last_error()
        assert f(n=0, r=None, t=None) == native.EINVAL   # an empty batch still needs its table
        assert f(n=0, r=None, s=8) == native.EINVAL
        assert f(n=0, r=None) == native.OK                # and touches nothing (the table is a fake address)
    assert bdev(r=rec + 8) == native.EINVAL
    assert "aligned" in native.last_error()
    assert bdev(t=tab + 4) == native.EINVAL
    assert bdev(n=0, r=None, t=tab + 4) == native.EINVAL
    for f in (wdev, whost):
        # the §14 parameter errors
        assert f(p=None) == native.EINVAL
        assert f(p=native.TimelineParams(0, 0, 4, 0)) == native.EINVAL
        assert "window_ns" in native.last_error()
        assert f(p=native.TimelineParams(0, 1000, 0, 0)) == native.EINVAL
        assert f(p=native.TimelineParams(0, 1000, 65537, 0)) == native.EINVAL
        assert f(p=native.TimelineParams(0, 1000, 4, 1)) == native.EINVAL
        assert f(s=8) == native.EINVAL
        assert "sub_bits" in native.last_error()
        assert f(o=None) == native.EINVAL
        assert f(a=None) == native.EINVAL
        assert f(r=None) == native.EINVAL
        assert f(n=big) == native.EINVAL
        assert f(n=0, a=None, r=None, o=None) == native.EINVAL
        assert f(n=0, a=None, r=None, p=native.TimelineParams(0, 0, 4, 0)) == native.EINVAL
        assert f(n=0, a=None, r=None) == native.OK
    assert wdev(r=rec + 8) == native.EINVAL
    assert "aligned" in native.last_error()
    assert wdev(a=arr + 4) == native.EINVAL
    assert wdev(o=tab + 4) == native.EINVAL


def test_python_rejects_before_the_library():
    recs = np.zeros(2, isim.REC_DTYPE)
    with pytest.raises(ValueError):
        isim.timeline_sketch_table(np.zeros(3, U64), recs, 1000, 4)
    with pytest.raises(ValueError):
        isim.latency_sketch(recs, 8)
    with pytest.raises(ValueError):
        isim.latency_sketch(recs, 3, out=np.zeros(991, U64))
    with pytest.raises(ValueError):
        isim.timeline_sketch_table(np.zeros(2, U64), recs, 1000, 4, sub_bits=3, out=np.zeros(992, U64))
    for bad in (0.9999999, 0.1234567, 1.0000001, -0.000001, 1.5):
        with pytest.raises(ValueError):
            isim.sketch_quantiles(3, np.zeros(992, U64), (0.5, bad))
        with pytest.raises(ValueError):
            isim.timeline_sketch(np.zeros(2, U64), recs, 1000, 4, q=(bad,))
        with pytest.raises(ValueError):
            isim.decode_timeline_sketch(np.zeros(6 * 992, U64), 4, 0, 1000, 3, (bad,))
    with pytest.raises(ValueError):
        isim.sketch_quantiles(3, np.zeros(991, U64))
    # the library's errors come through as IsimError
    with pytest.raises(isim.IsimError) as e:
        isim.timeline_sketch_device(0x10000, 0x20000, 2, 0, 4, d_out=0x30000)
    assert e.value.status == "EINVAL" and "window_ns" in str(e.value)
    with pytest.raises(isim.IsimError) as e:
        isim.latency_sketch_device(0x20000, 2, 9, d_table=0x30000)
    assert e.value.status == "EINVAL" and "sub_bits" in str(e.value)
    with pytest.raises(isim.IsimError):
        isim.sketch_bounds(3, 496)
    # empty batches need no GPU: nothing is touched
    assert not isim.latency_sketch(np.zeros(0, isim.REC_DTYPE), 3).any()
    assert isim.timeline_sketch_table(np.zeros(0, U64), np.zeros(0, isim.REC_DTYPE), 1000, 4, sub_bits=0).size == 6 * 130


def test_decode_hand_made_table():
    """2 windows of 1 s from t0 = 5 s at s = 3: rows before, w0, w1, after."""
    s, n_windows, t0, win, q = 3, 2, 5_000_000_000, 1_000_000_000, (0.5, 1.0)
    t = np.zeros((n_windows + 2, 2, py_bins(s)), U64)
    t[0] = _table(s, [(0, 7, 1)]).reshape(2, -1)
    t[1] = _table(s, [(0, 20, 2), (0, 40, 1), (1, 80, 1), (1, 9000, 1)]).reshape(2, -1)
    t[3] = _table(s, [(1, 11, 1), (1, MAXU, 1)]).reshape(2, -1)
    d = isim.decode_timeline_sketch(t.reshape(-1), n_windows, t0, win, s, q)
    B = lambda v: py_bounds(s, py_bucket(s, v))  # noqa: E731
    assert list(d["t_start_ns"]) == [5_000_000_000, 6_000_000_000] and d["q"] == q
    assert d["count"].shape == (3, 2) and d["count"].tolist() == [[5, 0], [3, 0], [2, 0]]
    assert d["lo_ns"].shape == d["hi_ns"].shape == (3, 2, 2) and d["lo_ns"].dtype == np.uint64
    pairs = lambda c, i, w: (int(d["lo_ns"][c, i, w]), int(d["hi_ns"][c, i, w]))  # noqa: E731
    assert pairs(native.Q_ALL, 0, 0) == B(40) and pairs(native.Q_ALL, 1, 0) == B(9000)
    assert pairs(native.Q_200, 0, 0) == B(20) and pairs(native.Q_200, 1, 0) == B(40)
    assert pairs(native.Q_500, 0, 0) == B(80) and pairs(native.Q_500, 1, 0) == B(9000)
    assert not d["lo_ns"][:, :, 1].any() and not d["hi_ns"][:, :, 1].any()
    assert d["before"]["count"].tolist() == [1, 1, 0]
    assert d["before"]["lo_ns"].tolist() == [[7, 7], [7, 7], [0, 0]] == d["before"]["hi_ns"].tolist()
    assert d["after"]["count"].tolist() == [2, 0, 2]
    assert d["after"]["lo_ns"].tolist() == [[11, B(MAXU)[0]], [0, 0], [11, B(MAXU)[0]]]
    assert d["after"]["hi_ns"].tolist() == [[11, MAXU], [0, 0], [11, MAXU]]


def test_python_surface():
    for name in ("sketch_bins", "sketch_bucket", "sketch_bounds", "sketch_words", "sketch_merge", "sketch_quantiles",
                 "latency_sketch", "latency_sketch_device", "timeline_sketch", "timeline_sketch_device",
                 "timeline_sketch_out_words", "timeline_sketch_table", "decode_timeline_sketch"):
        assert callable(getattr(isim, name)), name
    assert callable(isim.DesHandler.timeline_sketch)
