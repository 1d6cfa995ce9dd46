"""Per-service percentiles over time on the CPU: the header's constants and the sizes against
the formulae of include/isim.h; every argument the entry points refuse, found on the host before any HIP call;
the bindings; isim_service_window_quantiles_host against a restatement in Python integers (per cell and class,
sort each measure and take the nearest rank) and against the existing tables of the same spans: §28's
per-service table (one window that holds every finish; the counts summed over rows) and §23's FINISHED words."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import isim
from isim import native
from isim.quantiles import _ppm_array
from isim.service_window_quantiles import WAVE
from isim.yamljson import obj_to_json

from test_abi import declared_functions
from test_service_quantiles import hand_made, make_spans, nearest_rank, services

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "isim.h")).read()
M64 = (1 << 64) - 1
FUNCS = ["isim_service_window_quantiles_table_words", "isim_service_window_quantiles_workspace_bytes",
         "isim_service_window_quantiles_device", "isim_service_window_quantiles_host",
         "isim_service_window_quantiles"]
# (t0, window, n_windows): hand_made()'s finishes lie in 0 .. 2^40 + 2^33 + 2^20 and at 2^64 - 1
WINDOWS = {
    "three": (0, 1 << 39, 3),
    "late_t0": (1 << 39, (1 << 37) + 12345, 5),
    "one_ns": (7, 1, 4),
    "one_window": (3, 1 << 41, 1),
    "wraps": (M64 - 5, 1 << 63, 60),       # t0 + n_windows * W is far above 2^64
}


def params(t0, window, n_windows):
    return native.TimelineParams(t0, window, n_windows, 0)


def row_of(f, t0, window, n_windows):
    return 0 if f < t0 else 1 + min((f - t0) // window, n_windows)


def restate(spans, n_services, ppm, t0, window, n_windows):
    """The table in Python integers: (flat list of words, refused)."""
    ow, rows = 1 + len(ppm), n_windows + 2
    groups = {}
    folded = refused = 0
    for x in spans:
        a, s, f, svc, code = (int(x["arrival_ns"]), int(x["start_ns"]), int(x["finish_ns"]), int(x["service"]),
                              int(x["status"]) & 1)
        if svc >= n_services or not a <= s <= f:
            refused += 1
            continue
        folded += 1
        cell = svc * rows + row_of(f, t0, window, n_windows)
        for m, v in enumerate((s - a, f - s, f - a)):
            groups.setdefault((cell, m, 0), []).append(v)
            groups.setdefault((cell, m, 1 + code), []).append(v)
    flat = [0] * (n_services * rows * 9 * ow)
    for (cell, m, c), v in groups.items():
        v.sort()
        base = ((cell * 3 + m) * 3 + c) * ow
        flat[base:base + ow] = [len(v)] + [v[nearest_rank(len(v), p) - 1] for p in ppm]
    return flat + [folded, refused], refused


def host_table(h, spans, ppm, t0, window, n_windows):
    out = np.full(isim.service_window_quantiles_table_words(h, len(ppm), window, n_windows, t0), 0xAB, np.uint64)
    native.check(native.load().isim_service_window_quantiles_host(
        h._h, C.byref(params(t0, window, n_windows)), _ppm_array(ppm), len(ppm),
        spans.ctypes.data if len(spans) else None, len(spans), out.ctypes.data))
    return out


def test_constants_and_bindings():
    assert re.search(r"#define ISIM_SWQ_MAX_CELLS\s+\(1u << 20\)", HEADER) and native.SWQ_MAX_CELLS == 1 << 20
    m = re.search(r"#define ISIM_SWQ_WAVE\s+(\d+)", HEADER)
    assert m and int(m.group(1)) == native.SWQ_WAVE == WAVE and WAVE in (64, 128, 256)
    assert native.ABI_VERSION == 10
    go = open(os.path.join(ROOT, "go", "isim", "isim.go")).read()
    for fn in FUNCS:
        assert re.search(r"ISIM_API int %s\(" % fn, HEADER), fn
        assert fn in native.SIGNATURES, fn
        assert "C." + fn in go, fn
    assert set(declared_functions()) == set(native.SIGNATURES)
    assert isim.ServiceWindowQuantiles and isim.decode_service_window_quantiles


def pad256(x):
    return (x + 255) // 256 * 256


@pytest.mark.parametrize("ns,nw", [(1, 1), (13, 62), (300, 60), (1024, 1022)])
def test_sizes_follow_the_header_formulae(ns, nw):
    h = services(ns)
    cells = ns * (nw + 2)
    for n_q in (1, 5, 16):
        assert isim.service_window_quantiles_table_words(h, n_q, 1000, nw) == cells * 9 * (1 + n_q) + 2
        for cap in (0, 1, WAVE, WAVE + 1, 7 * (WAVE + 1) - 1, native.SVQ_STAGE + 1, 1 << 20, (1 << 32) - 1):
            mid = min(cells, cap // (WAVE + 1))
            slots = min(cells, cap // (native.SVQ_STAGE + 1))
            want = (256 + 3 * pad256(8 * cells) + pad256(4 * mid) + 24 * cap
                    + slots * (native.SVQ_SLOT_BYTES + 9 * n_q * 1024))
            assert isim.service_window_quantiles_workspace_bytes(h, cap, n_q, 1000, nw, 5) == want, (cap, n_q)


def _einval(rc, match):
    assert rc == native.EINVAL and match in native.last_error(), native.last_error()


def test_refusals_need_no_gpu():
    lib = native.load()
    items = services(3)
    static_doc = {"services": [{"name": "a", "isEntrypoint": True, "script": [{"sleep": "1ms"}, {"call": "b"}]},
                               {"name": "b", "script": [{"sleep": "1ms"}]}]}
    static = isim.Handler(isim.ServiceGraph.from_json(obj_to_json(static_doc)), None, isim.SimParams())
    buf = np.zeros(64, np.uint64)   # never dereferenced by a refused call
    a = buf.ctypes.data
    assert a % 16 == 0
    out = C.c_uint64()
    ok_q, bad_q = _ppm_array([500_000, 990_000]), _ppm_array([500_000, 1_000_001])
    ok_p = params(0, 1000, 4)

    def every(h, p, q, n_q, n=1):
        """Every entry point that takes the handler, the parameters and a quantile list."""
        hh = h._h if h is not None else None
        pp = C.byref(p) if p is not None else None
        return [lib.isim_service_window_quantiles_host(hh, pp, q, n_q, a, n, a),
                lib.isim_service_window_quantiles(0, hh, pp, q, n_q, a, n, a),
                lib.isim_service_window_quantiles_device(hh, pp, q, n_q, a, a, n, a, a, a, 1 << 40, None)]

    def sizes(h, p, n_q, cap=1):
        hh = h._h if h is not None else None
        pp = C.byref(p) if p is not None else None
        return [lib.isim_service_window_quantiles_table_words(hh, pp, n_q, C.byref(out)),
                lib.isim_service_window_quantiles_workspace_bytes(hh, pp, cap, n_q, C.byref(out))]

    for why, h, q, n_q in [("null handler", None, ok_q, 2), ("ISIM_FLAG_DYNAMIC", static, ok_q, 2),
                           ("n_q must be 1..16", items, ok_q, 0), ("n_q must be 1..16", items, ok_q, 17),
                           ("null q_ppm", items, None, 2), ("q_ppm[1] is above 1000000", items, bad_q, 2)]:
        for rc in every(h, ok_p, q, n_q):
            _einval(rc, why)
    for why, h, n_q in [("null handler", None, 2), ("ISIM_FLAG_DYNAMIC", static, 2), ("n_q must be 1..16", items, 0),
                        ("n_q must be 1..16", items, 17)]:
        for rc in sizes(h, ok_p, n_q):
            _einval(rc, why)
    # the parameter errors of isim_timeline, and the bound on the cells (below: 17 x 61681 is 2^20 + 1)
    for why, p in [("null isim_timeline_params", None), ("window_ns must be at least 1", params(0, 0, 4)),
                   ("n_windows must be 1..65536", params(0, 1000, 0)), ("n_windows must be 1..65536", params(0, 1000, 65537)),
                   ("reserved must be 0", native.TimelineParams(0, 1000, 4, 1))]:
        for rc in every(items, p, ok_q, 2) + sizes(items, p, 2):
            _einval(rc, why)
    for rc in every(services(17), params(0, 1000, 61679), ok_q, 2) + sizes(services(17), params(0, 1000, 61679), 2):
        _einval(rc, "above 2^20")
    assert sizes(services(17), params(0, 1000, 61678), 2) == [native.OK, native.OK]      # 17 x 61680 is 2^20 - 16
    for rc in every(items, ok_p, ok_q, 2, n=1 << 32):
        _einval(rc, "2^32 - 1")
    _einval(sizes(items, ok_p, 2, cap=1 << 32)[1], "2^32 - 1")
    _einval(lib.isim_service_window_quantiles_table_words(items._h, C.byref(ok_p), 2, None), "null")
    _einval(lib.isim_service_window_quantiles_workspace_bytes(items._h, C.byref(ok_p), 1, 2, None), "null")
    for call in (lambda *x: lib.isim_service_window_quantiles_host(items._h, C.byref(ok_p), ok_q, 2, *x),
                 lambda *x: lib.isim_service_window_quantiles(0, items._h, C.byref(ok_p), ok_q, 2, *x)):
        _einval(call(a, 1, None), "null table")
        _einval(call(None, 1, a), "null spans")
    _einval(lib.isim_service_window_quantiles_host(items._h, C.byref(ok_p), ok_q, 2, a, 1, a + 4), "aligned")

    need = isim.service_window_quantiles_workspace_bytes(items, 4, 2, 1000, 4)

    def dev(off=a, spans=a, cap=4, info=a, table=a, ws=a, ws_bytes=1 << 30):
        return lib.isim_service_window_quantiles_device(items._h, C.byref(ok_p), ok_q, 2, off, spans, cap, info, table,
                                                        ws, ws_bytes, None)

    for null in ("off", "info", "table", "spans"):
        _einval(dev(**{null: None}), "null")
    for mis in ("off", "info", "table", "ws"):
        _einval(dev(**{mis: a + 4}), "aligned")
    _einval(dev(spans=a + 8), "aligned")
    _einval(dev(ws_bytes=need - 1), "workspace")
    _einval(dev(ws=None), "workspace")
    with pytest.raises(isim.IsimError) as e:
        isim.DesHandler(static, 300_000).service_window_quantiles(0, 8)
    assert e.value.code == native.EINVAL


@pytest.mark.parametrize("name", list(WINDOWS))
@pytest.mark.parametrize("ppm", [[0, 1, 999_999, 1_000_000], [500_000], list(range(0, 1_000_001, 62_500))[:16]],
                         ids=["edges", "median", "sixteen"])
def test_host_equals_the_restatement(name, ppm):
    t0, window, nw = WINDOWS[name]
    spans, n_bad = hand_made()
    got = host_table(services(6), spans, ppm, t0, window, nw)
    want, refused = restate(spans, 6, ppm, t0, window, nw)
    assert refused == n_bad == int(got[-2 + native.SVQ_H_REFUSED])
    assert int(got[-2 + native.SVQ_H_FOLDED]) == len(spans) - n_bad
    assert [int(x) for x in got] == want
    cells, hdr = isim.decode_service_window_quantiles(got, 6, nw, len(ppm))
    assert np.array_equal(cells[:, :, 0, :, 0], cells[:, :, 1, :, 0]) and hdr["refused"] == n_bad
    assert int(cells[..., 0, 0, 0].sum()) == len(spans) - n_bad
    if name == "wraps":     # every finish but 2^64 - 1 is before t0, and that one opens window 0
        assert int(cells[:, 1, 0, 0, 0].sum()) == 3 == len(spans) - n_bad - int(cells[:, 0, 0, 0, 0].sum())


def edge_spans():
    """Finishes on a window's start, just before it, before t0, after the last window and at 2^64 - 1, for
    t0 = 100, W = 10, three windows."""
    rows = [(0, 0, f, 0, f & 1) for f in (0, 99, 100, 109, 110, 119, 120, 129, 130, 131, 1 << 40, M64)]
    return make_spans(rows)


def test_a_finish_on_a_window_start_opens_the_window():
    spans = edge_spans()
    t = host_table(services(1), spans, [1_000_000], 100, 10, 3)
    assert [int(x) for x in t] == restate(spans, 1, [1_000_000], 100, 10, 3)[0]
    cells, _ = isim.decode_service_window_quantiles(t, 1, 3, 1)
    assert [int(x) for x in cells[0, :, 2, 0, 0]] == [2, 2, 2, 2, 4]
    assert [int(x) for x in cells[0, :, 2, 0, 1]] == [99, 109, 119, 129, M64]


def test_against_the_other_tables_of_the_same_spans():
    spans, n_bad = hand_made()
    h = services(6)
    q = (0.0, 0.5, 0.99, 1.0)
    sq = isim.service_quantiles_host(h, spans, q)
    # one window that holds every finish below 2^63: drop the spans that end at 2^64 - 1 for this comparison
    low = spans[spans["finish_ns"] < (1 << 63)]
    one = isim.service_window_quantiles_host(h, low, q, 1 << 63, 1, 0)
    cells, hdr = isim.decode_service_window_quantiles(one, 6, 1, len(q))
    want, whdr = isim.decode_service_quantiles(isim.service_quantiles_host(h, low, q), 6, len(q))
    assert np.array_equal(cells[:, 1], want) and not cells[:, 0].any() and not cells[:, 2].any() and hdr == whdr
    # any windows: the class counts are §23's FINISHED words, and summed over the rows §28's counts
    for t0, window, nw in WINDOWS.values():
        flat = isim.service_window_quantiles_host(h, spans, q, window, nw, t0)
        cells, hdr = isim.decode_service_window_quantiles(flat, 6, nw, len(q))
        tl = isim.service_timeline_host(h, spans, window, nw, t0)
        rows = tl[:-native.SVT_ROW_WORDS].reshape(6, nw + 2, native.SVT_ROW_WORDS)
        for code, cls in ((0, native.Q_200), (1, native.Q_500)):
            assert np.array_equal(cells[:, :, 0, cls, 0], rows[:, :, native.SVT_FINISHED + code])
        total, _ = isim.decode_service_quantiles(sq, 6, len(q))
        assert np.array_equal(cells[:, :, :, :, 0].sum(axis=1), total[:, :, :, 0])
        assert hdr["refused"] == n_bad == int(tl[-native.SVT_ROW_WORDS + native.SVT_H_REFUSED])


def test_the_python_view():
    spans, n_bad = hand_made()
    h = services(6)
    q = (0.5, 0.99, 1.0)
    t0, window, nw = WINDOWS["three"]
    wq = isim.ServiceWindowQuantiles(h, q, window, nw, t0, isim.service_window_quantiles_host(h, spans, q, window, nw, t0))
    assert wq.header["refused"] == n_bad and wq.cells.shape == (6, 5, 3, 3, 4)
    assert wq.counts["all"].shape == (6, 5) and wq.values["duration"]["500"].shape == (6, 5, 3)
    assert int(wq.counts["all"].sum()) == len(spans) - n_bad
    s = wq.series("s5", "duration", 0.99)
    assert s.shape == (5,) and np.array_equal(s, wq.series(5, "duration", 0.99)) and np.array_equal(s, wq.cells[5, :, 2, 0, 2])
    worst = wq.worst("wait", 1.0, 2)
    assert worst[0] == ("s3", 4, M64) and len(worst) == 2         # (0, 2^64 - 1, 2^64 - 1) finishes "after"
    assert all(int(wq.counts["500"][int(n[1:]), r]) for n, r, _ in wq.worst("service", 0.5, 50, cls="500"))
    text = wq.to_text(top=3).splitlines()
    assert len(text) == 5 and text[0].startswith(f"service window quantiles of {len(spans) - n_bad} spans")
    assert "wait p50" in text[1] and "dur p100" in text[1] and "row" in text[1]
