"""Per-service percentiles on the CPU: the header's constants and the sizes against the
formulae of include/isim.h; every argument the entry points refuse, found on the host before any HIP call;
the bindings; isim_service_quantiles_host against hand-derived vectors and against a restatement in Python
integers (per service and class, sort each measure and take the nearest rank)."""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest

import isim
from isim import native
from isim.quantiles import _ppm_array
from isim.service_quantiles import CHUNK, STAGE
from isim.yamljson import obj_to_json, yaml_to_json

from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "isim.h")).read()
KAT = os.path.join(ROOT, "tests", "golden", "service_quantiles_kat.json")
M64 = (1 << 64) - 1
FUNCS = ["isim_service_quantiles_table_words", "isim_service_quantiles_workspace_bytes",
         "isim_service_quantiles_device", "isim_service_quantiles_host", "isim_service_quantiles"]


@functools.lru_cache(maxsize=None)
def services(n):
    """A handler of n services on the item engine; only the services' number matters to the select."""
    doc = {"services": [{"name": f"s{i}", "isEntrypoint": i == 0} for i in range(n)]}
    return isim.Handler(isim.ServiceGraph.from_json(obj_to_json(doc)), None, isim.SimParams(flags=native.FLAG_DYNAMIC))


def make_spans(rows):
    """[(a, S, F, service, status)] as isim_des_span records."""
    out = np.zeros(len(rows), isim.DES_SPAN_DTYPE)
    for i, (a, s, f, svc, st) in enumerate(rows):
        out[i]["arrival_ns"], out[i]["start_ns"], out[i]["finish_ns"] = a, s, f
        out[i]["service"], out[i]["status"] = svc, st
    return out


def nearest_rank(n, ppm):
    return max(1, -(-ppm * n // 1_000_000))


def restate(spans, n_services, ppm):
    """The table in Python integers: (flat list of words, refused)."""
    ow = 1 + len(ppm)
    cells = [[[[0] * ow for _ in range(3)] for _ in range(3)] for _ in range(n_services)]
    groups = [[[[] for _ in range(3)] for _ in range(3)] for _ in range(n_services)]   # [service][measure][class]
    folded = refused = 0
    for x in spans:
        a, s, f, svc, code = int(x["arrival_ns"]), int(x["start_ns"]), int(x["finish_ns"]), int(x["service"]), int(x["status"]) & 1
        if svc >= n_services or not a <= s <= f:
            refused += 1
            continue
        folded += 1
        for m, v in enumerate((s - a, f - s, f - a)):
            groups[svc][m][0].append(v)
            groups[svc][m][1 + code].append(v)
    for svc in range(n_services):
        for m in range(3):
            for c in range(3):
                v = sorted(groups[svc][m][c])
                if v:
                    cells[svc][m][c] = [len(v)] + [v[nearest_rank(len(v), p) - 1] for p in ppm]
    flat = [w for s in cells for m in s for c in m for w in c] + [folded, refused]
    return flat, refused


def host_table(h, spans, ppm):
    out = np.full(isim.service_quantiles_table_words(h, len(ppm)), 0xAB, np.uint64)   # dirty
    native.check(native.load().isim_service_quantiles_host(h._h, _ppm_array(ppm), len(ppm),
                                                           spans.ctypes.data if len(spans) else None, len(spans),
                                                           out.ctypes.data))
    return out


def test_constants_match_the_header():
    for name in ("WAIT", "SERVICE", "DURATION", "MEASURES", "CLASSES", "H_FOLDED", "H_REFUSED", "HEADER_WORDS",
                 "STAGE", "CHUNK", "SLOT_BYTES"):
        m = re.search(r"#define ISIM_SVQ_%s\s+(\d+)" % name, HEADER)
        assert m and int(m.group(1)) == getattr(native, "SVQ_" + name), name
    assert re.search(r"#define ISIM_SVQ_MAX_SPANS\s+0xFFFFFFFFull", HEADER) and native.SVQ_MAX_SPANS == (1 << 32) - 1
    assert (native.SVQ_WAIT, native.SVQ_SERVICE, native.SVQ_DURATION) == (0, 1, 2)
    assert native.SVQ_MEASURES == native.SVQ_CLASSES == 3 and native.SVQ_HEADER_WORDS == 2
    assert STAGE == native.SVQ_STAGE and CHUNK == native.SVQ_CHUNK
    assert isim.MEASURE_NAMES == ("wait", "service", "duration")
    assert native.ABI_VERSION == 10


def test_bindings_declare_the_new_functions():
    go = open(os.path.join(ROOT, "go", "isim", "isim.go")).read()
    for fn in FUNCS:
        assert re.search(r"ISIM_API int %s\(" % fn, HEADER), fn
        assert fn in native.SIGNATURES, fn
    for fn in ("isim_service_quantiles_table_words", "isim_service_quantiles_host", "isim_service_quantiles"):
        assert "C." + fn + "(" in go, fn
    assert set(declared_functions()) == set(native.SIGNATURES)


def pad256(x):
    return (x + 255) // 256 * 256


@pytest.mark.parametrize("ns", [1, 13, 300])
def test_sizes_follow_the_header_formulae(ns):
    h = services(ns)
    for n_q in (1, 5, 16):
        assert isim.service_quantiles_table_words(h, n_q) == ns * 9 * (1 + n_q) + 2
        for cap in (0, 1, native.SVQ_STAGE, native.SVQ_STAGE + 1, 10 * (native.SVQ_STAGE + 1) - 1, 1 << 20, (1 << 32) - 1):
            slots = min(ns, cap // (native.SVQ_STAGE + 1))
            want = 256 + 3 * pad256(8 * ns) + 24 * cap + slots * (native.SVQ_SLOT_BYTES + 9 * n_q * 1024)
            assert isim.service_quantiles_workspace_bytes(h, cap, n_q) == want, (cap, n_q)


def _einval(rc, match):
    assert rc == native.EINVAL and match in native.last_error(), native.last_error()


def test_refusals_need_no_gpu():
    lib = native.load()
    items = services(3)
    static_doc = {"services": [{"name": "a", "isEntrypoint": True, "script": [{"sleep": "1ms"}, {"call": "b"}]},
                               {"name": "b", "script": [{"sleep": "1ms"}]}]}
    static = isim.Handler(isim.ServiceGraph.from_json(obj_to_json(static_doc)), None, isim.SimParams())
    canonical = yaml_to_json(open(os.path.join(ROOT, "tests", "golden", "topologies", "canonical.yaml"), "rb").read())
    dag = isim.Handler(isim.ServiceGraph.from_json(canonical), None,
                       isim.SimParams(flags=native.FLAG_DYNAMIC | native.FLAG_TREE_DAG))   # walks the site graph: no tap
    buf = np.zeros(64, np.uint64)   # never dereferenced by a refused call
    a = buf.ctypes.data
    assert a % 16 == 0
    out = C.c_uint64()
    ok_q, bad_q = _ppm_array([500_000, 990_000]), _ppm_array([500_000, 1_000_001])

    def every(h, q, n_q, n=1):
        """Every entry point that takes the handler and a quantile list."""
        hh = h._h if h is not None else None
        return [lib.isim_service_quantiles_host(hh, q, n_q, a, n, a),
                lib.isim_service_quantiles(0, hh, q, n_q, a, n, a),
                lib.isim_service_quantiles_device(hh, q, n_q, a, a, n, a, a, a, 1 << 40, None)]

    def sizes(h, n_q, cap=1):
        hh = h._h if h is not None else None
        return [lib.isim_service_quantiles_table_words(hh, n_q, C.byref(out)),
                lib.isim_service_quantiles_workspace_bytes(hh, cap, n_q, C.byref(out))]

    for why, h, q, n_q in [("null handler", None, ok_q, 2), ("ISIM_FLAG_DYNAMIC", static, ok_q, 2),
                           ("site graph", dag, ok_q, 2),
                           ("n_q must be 1..16", items, ok_q, 0), ("n_q must be 1..16", items, ok_q, 17),
                           ("null q_ppm", items, None, 2), ("q_ppm[1] is above 1000000", items, bad_q, 2)]:
        for rc in every(h, q, n_q):
            _einval(rc, why)
    for why, h, n_q in [("null handler", None, 2), ("ISIM_FLAG_DYNAMIC", static, 2), ("site graph", dag, 2),
                        ("n_q must be 1..16", items, 0),
                        ("n_q must be 1..16", items, 17)]:
        for rc in sizes(h, n_q):
            _einval(rc, why)
    for rc in every(items, ok_q, 2, n=1 << 32):
        _einval(rc, "2^32 - 1")
    _einval(sizes(items, 2, cap=1 << 32)[1], "2^32 - 1")
    _einval(lib.isim_service_quantiles_table_words(items._h, 2, None), "null")
    _einval(lib.isim_service_quantiles_workspace_bytes(items._h, 1, 2, None), "null")
    for call in (lambda *x: lib.isim_service_quantiles_host(items._h, ok_q, 2, *x),
                 lambda *x: lib.isim_service_quantiles(0, items._h, ok_q, 2, *x)):
        _einval(call(a, 1, None), "null table")
        _einval(call(None, 1, a), "null spans")
    _einval(lib.isim_service_quantiles_host(items._h, ok_q, 2, a, 1, a + 4), "aligned")

    need = isim.service_quantiles_workspace_bytes(items, 4, 2)

    def dev(off=a, spans=a, cap=4, info=a, table=a, ws=a, ws_bytes=1 << 30):
        return lib.isim_service_quantiles_device(items._h, ok_q, 2, off, spans, cap, info, table, ws, ws_bytes, None)

    for null in ("off", "info", "table", "spans"):
        _einval(dev(**{null: None}), "null")
    for mis in ("off", "info", "table", "ws"):
        _einval(dev(**{mis: a + 4}), "aligned")
    _einval(dev(spans=a + 8), "aligned")
    _einval(dev(ws_bytes=need - 1), "workspace")
    _einval(dev(ws=None), "workspace")
    with pytest.raises(isim.IsimError) as e:
        isim.DesHandler(static, 300_000).service_quantiles(0, 8)
    assert e.value.code == native.EINVAL
    with pytest.raises(ValueError):
        isim.service_quantiles_host(items, make_spans([]), q=(0.5000001,))


def kat_cases():
    return json.load(open(KAT))["cases"]


@pytest.mark.parametrize("case", kat_cases(), ids=[c["name"] for c in kat_cases()])
def test_hand_derived_vectors(case):
    ns, ppm = case["n_services"], case["q_ppm"]
    ow = 1 + len(ppm)
    want = [0] * (ns * 9 * ow + 2)
    for svc, m, c, *words in case["cells"]:
        base = ((svc * 3 + m) * 3 + c) * ow
        want[base:base + ow] = words
    want[-2:] = case["header"]
    spans = make_spans(case["spans"])
    got = host_table(services(ns), spans, ppm)
    assert [int(x) for x in got] == want
    assert restate(spans, ns, ppm)[0] == want


def hand_made():
    """Six services: none, N = 1, all equal, 0 and 2^64 - 1 in one segment, 500s only, a few hundred random; with
    refused spans planted between them."""
    rng = np.random.default_rng(28)
    rows = [(10, 12, 20, 1, 0)]
    rows += [(5, 7, 12, 2, i & 1) for i in range(10)]
    rows += [(0, 0, 0, 3, 0), (0, M64, M64, 3, 0), (0, 0, M64, 3, 1), (M64, M64, M64, 3, 1), (7, 7, 9, 3, 0)]
    rows += [(i, i + 3 * i, 5 * i + 1, 4, 1) for i in range(1, 40)]
    for _ in range(700):
        a = int(rng.integers(0, 1 << 40))
        w = int(rng.integers(0, 50)) if rng.random() < 0.7 else int(rng.integers(0, 1 << 33))
        d = int(rng.integers(0, 1 << 20))
        rows.append((a, a + w, a + w + d, 5, int(rng.random() < 0.2) | (int(rng.random() < 0.5) << 1)))
    bad = [(3, 2, 9, 1, 0), (1, 5, 4, 2, 0), (0, 0, 0, 6, 0), (0, 0, 0, 0xFFFFFFFF, 1), (M64, 0, 5, 5, 0),
           (5, 5, 4, 0, 0), (9, 8, M64, 3, 1)]
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    for i, b in enumerate(bad):
        rows.insert(11 * i, b)
    return make_spans(rows), len(bad)


@pytest.mark.parametrize("ppm", [[0, 1, 999_999, 1_000_000], [500_000], list(range(0, 1_000_001, 62_500))[:16]],
                         ids=["edges", "median", "sixteen"])
def test_host_equals_the_restatement(ppm):
    spans, n_bad = hand_made()
    got = host_table(services(6), spans, ppm)
    want, refused = restate(spans, 6, ppm)
    assert refused == n_bad == int(got[-2 + native.SVQ_H_REFUSED])
    assert int(got[-2 + native.SVQ_H_FOLDED]) == len(spans) - n_bad
    assert [int(x) for x in got] == want
    cells, hdr = isim.decode_service_quantiles(got, 6, len(ppm))
    assert not cells[0].any() and int(cells[1, 0, 0, 0]) == 1 and int(cells[4, 0, 1, 0]) == 0     # none, N = 1, 500s only
    assert np.array_equal(cells[:, 0, :, 0], cells[:, 1, :, 0]) and np.array_equal(cells[:, 0, :, 0], cells[:, 2, :, 0])
    assert hdr == {"folded": len(spans) - n_bad, "refused": n_bad}


def test_the_python_view():
    spans, n_bad = hand_made()
    h = services(6)
    q = (0.5, 0.99, 1.0)
    flat = isim.service_quantiles_host(h, spans, q)
    sq = isim.ServiceQuantiles(h, q, flat)
    assert sq.header["refused"] == n_bad and sq.names == [f"s{i}" for i in range(6)]
    assert list(sq.counts["all"]) == [0, 1, 10, 5, 39, 700] and int(sq.counts["200"][4]) == 0
    assert sq.values["duration"]["all"].shape == (6, 3)
    worst = sq.worst("wait", 1.0, 2)
    assert worst[0] == ("s3", M64) and len(worst) == 2
    assert all(name != "s0" for name, _ in sq.worst("duration", 0.5, 6)) and len(sq.worst("duration", 0.5, 6)) == 5
    # values above 2^53 that differ in their low bits only are still ordered by value
    big = flat.copy()
    cells, _ = isim.decode_service_quantiles(big, 6, 3)
    cells[1, 2, 0, 1:], cells[2, 2, 0, 1:], cells[4, 2, 0, 1:] = (1 << 60) + 1, (1 << 60) + 3, (1 << 60) + 2
    assert [n for n, _ in isim.ServiceQuantiles(h, q, big).worst("duration", 0.5, 3)] == ["s2", "s4", "s1"]
    text = sq.to_text(top=3).splitlines()
    assert len(text) == 5 and text[0].startswith(f"service quantiles of {len(spans) - n_bad} spans")
    assert "wait p50" in text[1] and "dur p100" in text[1]
