"""Exact latency percentiles (include/isim.h isim_latency_quantiles*, DESIGN.md
§13), the host side: the nearest-rank rule, the workspace size, argument
checks that need no device memory, and the Python wrapper's ppm conversion.
The select itself runs on the GPU: tests/test_quantiles_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import isim
from isim import native, quantiles

NS = [1, 2, 3, 999, 1000, 1001, 10**6, 1 << 40]
PPMS = [0, 1, 499999, 500000, 500001, 990000, 999000, 999999, 1000000]


def rank(n, q_ppm):
    """The nearest-rank rule restated: k = max(1, ceil(q_ppm * n / 1e6)), in exact integers."""
    return max(1, -((-q_ppm * n) // 10**6))


def c_rank(n, q_ppm):
    k = C.c_uint64(0xDEAD)
    rc = native.load().isim_quantile_rank(n, q_ppm, C.byref(k))
    return rc, int(k.value)


@pytest.mark.parametrize("n", NS)
def test_rank_matches_the_rule(n):
    for q in PPMS:
        assert c_rank(n, q) == (native.OK, rank(n, q)), (n, q)
        assert isim.quantile_rank(n, q) == rank(n, q)
    assert c_rank(n, 0) == (native.OK, 1)
    assert c_rank(n, 1000000) == (native.OK, n)


def test_rank_rejects_bad_arguments():
    for n, q in ((0, 500000), ((1 << 40) + 1, 500000), (10, 1000001)):
        rc, _ = c_rank(n, q)
        assert rc == native.EINVAL and native.last_error(), (n, q)
    assert native.load().isim_quantile_rank(10, 5, None) == native.EINVAL
    with pytest.raises(isim.IsimError) as e:
        isim.quantile_rank(0, 1)
    assert e.value.code == native.EINVAL


def test_workspace_size():
    sizes = [isim.quantiles_workspace_bytes(n_q) for n_q in range(1, native.MAX_QUANTILES + 1)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    assert 0 < sizes[0] and sizes[-1] <= 300 * 1024
    assert all(s % 8 == 0 for s in sizes)
    b = C.c_uint64()
    for n_q in (0, native.MAX_QUANTILES + 1):
        assert native.load().isim_quantiles_workspace_bytes(n_q, C.byref(b)) == native.EINVAL
        assert native.last_error()
    assert native.load().isim_quantiles_workspace_bytes(1, None) == native.EINVAL
    assert isim.quantiles_out_words(5) == 18


# pointers that are never dereferenced: every case below fails its argument check first
FAKE_REC, FAKE_OUT, FAKE_WS = 0x10000, 0x20000, 0x30000


def _device_call(d_records=FAKE_REC, n=100, ppm=(500000,), n_q=None, d_out=FAKE_OUT, d_ws=FAKE_WS, ws_bytes=None):
    n_q = len(ppm) if n_q is None else n_q
    arr = (C.c_uint32 * max(1, len(ppm)))(*ppm)
    if ws_bytes is None:
        ws_bytes = isim.quantiles_workspace_bytes(max(1, min(n_q, native.MAX_QUANTILES)))
    return native.load().isim_latency_quantiles_device(d_records, n, arr, n_q, d_out, d_ws, ws_bytes, None)


@pytest.mark.parametrize("case,kw", [
    ("n_q 0", dict(ppm=(), n_q=0)),
    ("n_q above 16", dict(ppm=(1,) * 17)),
    ("q_ppm above 10^6", dict(ppm=(500000, 1000001))),
    ("n_records above 2^40", dict(n=(1 << 40) + 1)),
    ("workspace too small", dict(ws_bytes=isim.quantiles_workspace_bytes(1) - 1)),
    ("workspace sized for fewer quantiles", dict(ppm=(1, 2, 3), ws_bytes=isim.quantiles_workspace_bytes(2))),
    ("null d_out", dict(d_out=None)),
    ("null d_workspace", dict(d_ws=None)),
    ("records not 16-byte aligned", dict(d_records=FAKE_REC + 8)),
])
def test_device_call_einval(case, kw):
    native.load().isim_quantile_rank(1, 1, None)  # leaves another message behind
    before = native.last_error()
    assert _device_call(**kw) == native.EINVAL, case
    assert native.last_error() and native.last_error() != before, case


@pytest.mark.parametrize("case,ppm,n_q,null_out", [
    ("n_q 0", (), 0, False),
    ("n_q above 16", (1,) * 17, 17, False),
    ("q_ppm above 10^6", (1000001,), 1, False),
    ("null h_out", (500000,), 1, True),
])
def test_host_call_einval(case, ppm, n_q, null_out):
    recs = np.zeros(4, isim.REC_DTYPE)
    out = np.zeros(isim.quantiles_out_words(max(1, n_q)), np.uint64)
    arr = (C.c_uint32 * max(1, len(ppm)))(*ppm)
    rc = native.load().isim_latency_quantiles(0, recs.ctypes.data, len(recs), arr, n_q,
                                              None if null_out else out.ctypes.data)
    assert rc == native.EINVAL and native.last_error(), case


def test_python_wrapper_ppm():
    assert quantiles.q_to_ppm([0.999]) == [999000]
    assert quantiles.q_to_ppm(isim.DEFAULT_Q) == [500000, 750000, 900000, 990000, 999000]
    assert quantiles.q_to_ppm([0, 1, 0.000001]) == [0, 1000000, 1]
    for bad in (0.1234567, -0.1, 1.000001, 0.9999999):
        with pytest.raises(ValueError):
            quantiles.q_to_ppm([bad])
    recs = np.zeros(4, isim.REC_DTYPE)
    with pytest.raises(ValueError):
        isim.latency_quantiles(recs, q=(0.1234567,))
    with pytest.raises(ValueError):
        isim.latency_quantiles_device(FAKE_REC, 4, q=(0.1234567,), d_out=FAKE_OUT, d_workspace=FAKE_WS)
    # accepted by the wrapper: the call then reaches libisim's own checks (a misaligned records pointer)
    with pytest.raises(isim.IsimError) as e:
        isim.latency_quantiles_device(FAKE_REC + 4, 4, q=(0.999,), d_out=FAKE_OUT, d_workspace=FAKE_WS)
    assert e.value.code == native.EINVAL and "aligned" in str(e.value)


def test_decode_layout():
    out = np.arange(3 * 3, dtype=np.uint64)
    d = quantiles.decode_quantiles(out, (0.5, 0.99))
    assert d == {"all": {"count": 0, "q": {0.5: 1, 0.99: 2}}, "200": {"count": 3, "q": {0.5: 4, 0.99: 5}},
                 "500": {"count": 6, "q": {0.5: 7, 0.99: 8}}}
    assert (native.Q_ALL, native.Q_200, native.Q_500) == (0, 1, 2) and native.MAX_QUANTILES == 16
