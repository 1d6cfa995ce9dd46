"""The per-service latency sketch on the CPU: the declarations against the bindings; the sizes
against the formulae of include/isim.h; isim_service_sketch_host word for word against a restatement in
Python integers (the refusal rule, three measures, the bucket rule, a count per word); accumulation, the merge
and the brackets against isim_sketch_quantiles, against isim_service_quantiles_host's exact values and against
order statistics sorted in Python; every argument the entry points refuse, found on the host before any HIP
call; the Python view."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import isim
from isim import native
from isim.quantiles import _ppm_array
from isim.service_sketch import SHORT, ServiceSketch
from isim.yamljson import obj_to_json, yaml_to_json

from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "isim.h")).read()
M64 = (1 << 64) - 1
FUNCS = ["isim_service_sketch_table_words", "isim_service_sketch_workspace_bytes", "isim_service_sketch_merge",
         "isim_service_sketch_quantiles", "isim_service_sketch_device", "isim_service_sketch_host",
         "isim_service_sketch"]
SUB_BITS = [0, 3, 7]


@functools.lru_cache(maxsize=None)
def services(n):
    """A handler of n services on the item engine; only the services' number matters to the sketch."""
    doc = {"services": [{"name": f"s{i}", "isEntrypoint": i == 0} for i in range(n)]}
    return isim.Handler(isim.ServiceGraph.from_json(obj_to_json(doc)), None, isim.SimParams(flags=native.FLAG_DYNAMIC))


def make_spans(rows):
    """[(a, S, F, service, status)] as isim_des_span records."""
    out = np.zeros(len(rows), isim.DES_SPAN_DTYPE)
    for i, (a, s, f, svc, st) in enumerate(rows):
        out[i]["arrival_ns"], out[i]["start_ns"], out[i]["finish_ns"] = a, s, f
        out[i]["service"], out[i]["status"] = svc, st
    return out


def bins_of(s):
    return (65 - s) << s


def bucket(s, v):
    """The bucket rule of isim.h in Python integers."""
    if v < (2 << s):
        return v
    shift = v.bit_length() - (s + 1)
    return (shift << s) + (v >> shift)


def restate(spans, n_services, s):
    """The table of one fold into zeros, in Python integers."""
    bins = bins_of(s)
    t = [0] * (n_services * 3 * 2 * bins + 2)
    for x in spans:
        a, st, f, svc, code = int(x["arrival_ns"]), int(x["start_ns"]), int(x["finish_ns"]), int(x["service"]), int(x["status"]) & 1
        if svc >= n_services or not a <= st <= f:
            t[-2 + native.SVQ_H_REFUSED] += 1
            continue
        t[-2 + native.SVQ_H_FOLDED] += 1
        for m, v in enumerate((st - a, f - st, f - a)):
            t[((svc * 3 + m) * 2 + code) * bins + bucket(s, v)] += 1
    return t


def host_fold(h, spans, s, out=None):
    return isim.service_sketch_host(h, spans, s, out=out)


def test_constants_and_declarations():
    m = re.search(r"#define ISIM_SVS_SHORT\s+(\d+)", HEADER)
    assert m and int(m.group(1)) == native.SVS_SHORT == SHORT
    assert re.search(r"#define ISIM_SVS_MAX_WORDS\s+\(1ull << 32\)", HEADER) and native.SVS_MAX_WORDS == 1 << 32
    assert 1 <= native.SVS_SHORT <= native.SVQ_CHUNK
    assert native.ABI_VERSION == 10 and re.search(r"#define ISIM_ABI_VERSION 10\b", HEADER)
    for fn in FUNCS:
        assert re.search(r"ISIM_API int %s\(" % fn, HEADER), fn
        assert fn in native.SIGNATURES, fn
    assert set(declared_functions()) == set(native.SIGNATURES)
    assert 100_000 * 6 * bins_of(3) + 2 < native.SVS_MAX_WORDS      # what the bound is said to admit


def pad256(x):
    return (x + 255) // 256 * 256


@pytest.mark.parametrize("ns", [1, 13, 300])
def test_sizes_follow_the_header_formulae(ns):
    h = services(ns)
    for s in range(8):
        assert isim.service_sketch_table_words(h, s) == ns * 3 * 2 * native.SK_BINS(s) + native.SVQ_HEADER_WORDS
    T = native.SVS_SHORT
    for cap in (0, 1, T, T + 1, 10 * (T + 1) - 1, 1 << 20, (1 << 32) - 1):
        want = 256 + 3 * pad256(8 * ns) + 24 * cap + min(ns, cap // (T + 1)) * native.SVQ_SLOT_BYTES
        assert isim.service_sketch_workspace_bytes(h, cap) == want, cap


def edge_spans(s):
    """Five services: none (0); one span (1); 200s only with the bucket rule's edges in every measure (2); 500s
    only, a = 0 and F = 2^64 - 1 (3); a few hundred random (4); every kind of refused span between them."""
    rng = np.random.default_rng(30)
    e = (2 << s)
    rows = [(10, 12, 20, 1, 0)]
    for v in (0, e - 1, e, e + 1, M64):
        rows += [(0, v, v, 2, 0), (0, 0, v, 2, 2), (7, 7, 7 + min(v, M64 - 7), 2, 0)]
    rows += [(0, 0, M64, 3, 1), (0, M64, M64, 3, 3), (0, 1, M64, 3, 1), (M64, M64, M64, 3, 1)]
    for _ in range(400):
        a = int(rng.integers(0, 1 << 40))
        w = int(rng.integers(0, 50)) if rng.random() < 0.7 else int(rng.integers(0, 1 << 33))
        d = int(rng.integers(0, 1 << 20))
        rows.append((a, a + w, a + w + d, 4, int(rng.random() < 0.2) | (int(rng.random() < 0.5) << 1)))
    bad = [(3, 2, 9, 1, 0), (1, 5, 4, 2, 0), (0, 0, 0, 5, 0), (0, 0, 0, 0xFFFFFFFF, 1), (M64, 0, 5, 4, 0),
           (5, 5, 4, 0, 0), (9, 8, M64, 3, 1)]   # S < a, F < S, service >= n (twice), S < a, F < S, S < a
    rows = [rows[i] for i in rng.permutation(len(rows))]
    for i, b in enumerate(bad):
        rows.insert(11 * i, b)
    return make_spans(rows), len(bad)


@pytest.mark.parametrize("s", SUB_BITS)
def test_host_equals_the_restatement(s):
    h = services(5)
    spans, n_bad = edge_spans(s)
    got = host_fold(h, spans, s)
    want = restate(spans, 5, s)
    assert [int(x) for x in got] == want
    assert int(got[-2 + native.SVQ_H_REFUSED]) == n_bad and int(got[-2 + native.SVQ_H_FOLDED]) == len(spans) - n_bad
    sk = isim.ServiceSketch(h, s, got)
    assert not sk.blocks[0].any()                                                        # no span
    assert [int(sk.blocks[1, m].sum()) for m in range(3)] == [1, 1, 1]                   # one span
    assert not sk.blocks[2, :, 1].any() and not sk.blocks[3, :, 0].any()                 # 200s only, 500s only
    assert int(sk.blocks[3, 2, 1, -1]) == 3                                              # 2^64 - 1: the last bin
    # empty input and one span alone
    assert not host_fold(h, make_spans([]), s).any()
    one = host_fold(h, make_spans([(10, 12, 20, 1, 1)]), s)
    assert int(one.sum()) == 4 and [int(x) for x in one] == restate(make_spans([(10, 12, 20, 1, 1)]), 5, s)


@pytest.mark.parametrize("s", SUB_BITS)
def test_two_calls_equal_twice_one_call_and_the_merge_adds_every_word(s):
    h = services(5)
    spans, _ = edge_spans(s)
    once = host_fold(h, spans, s)
    twice = host_fold(h, spans, s, out=once.copy())
    assert np.array_equal(twice, 2 * once) and int(twice[-2]) == 2 * int(once[-2])
    other = host_fold(h, spans[::3], s)
    dst = once.copy()
    assert isim.service_sketch_merge(h, s, dst, other) is dst
    assert np.array_equal(dst, once + other) and int(dst[-1]) == int(once[-1]) + int(other[-1])
    a, b = isim.ServiceSketch(h, s, once.copy()), isim.ServiceSketch(h, s, other)
    assert a.merge(b) is a and np.array_equal(a.flat, dst) and a.header["folded"] == int(dst[-2])
    with pytest.raises(ValueError):
        a.merge(isim.ServiceSketch(h, s ^ 1))
    # the split of a list over two calls is the fold of the whole list
    halves = host_fold(h, spans[len(spans) // 2:], s, out=host_fold(h, spans[:len(spans) // 2], s))
    assert np.array_equal(halves, once)


@pytest.mark.parametrize("s", SUB_BITS)
def test_quantiles_are_those_of_each_block(s):
    h = services(5)
    spans, _ = edge_spans(s)
    table = host_fold(h, spans, s)
    ppm = [0, 500_000, 990_000, 1_000_000]
    got = isim.service_sketch_quantiles(h, s, table, [p / 1e6 for p in ppm])
    assert got.shape == (5, 3, 3, 1 + 2 * len(ppm))
    lib, bw = native.load(), native.SK_WORDS(s)
    for b in range(15):
        want = np.zeros(native.SKQ_OUT_WORDS(len(ppm)), np.uint64)
        native.check(lib.isim_sketch_quantiles(s, table[b * bw:].ctypes.data, _ppm_array(ppm), len(ppm), want.ctypes.data))
        assert np.array_equal(got[b // 3, b % 3].ravel(), want), b


@pytest.mark.parametrize("s", SUB_BITS)
def test_brackets_contain_the_exact_per_service_values(s):
    h = services(5)
    spans, _ = edge_spans(s)
    q = (0.0, 0.5, 0.9, 0.99, 1.0)
    exact, _ = isim.decode_service_quantiles(isim.service_quantiles_host(h, spans, q), 5, len(q))
    br = isim.service_sketch_quantiles(h, s, host_fold(h, spans, s), q)
    for svc in range(5):
        for m in range(3):
            for c in range(3):
                assert int(br[svc, m, c, 0]) == int(exact[svc, m, c, 0])
                for i in range(len(q)):
                    lo, hi, v = int(br[svc, m, c, 1 + 2 * i]), int(br[svc, m, c, 2 + 2 * i]), int(exact[svc, m, c, 1 + i])
                    assert lo <= v <= hi and hi - lo < max(1, lo >> s), (svc, m, c, i, lo, v, hi)


def nearest_rank(n, ppm):
    return max(1, -(-ppm * n // 1_000_000))


@pytest.mark.parametrize("s", SUB_BITS)
def test_two_lists_in_one_table_bracket_the_concatenation(s):
    h = services(5)
    first, _ = edge_spans(s)
    rng = np.random.default_rng(31)
    second = make_spans([(a, a + int(rng.integers(0, 1 << 30)), a + (1 << 30) + int(rng.integers(0, 1 << 35)),
                          int(rng.integers(1, 5)), int(rng.integers(0, 2))) for a in range(0, 6000, 20)])
    table = host_fold(h, second, s, out=host_fold(h, first, s))
    ppm = [0, 250_000, 500_000, 999_000, 1_000_000]
    br = isim.service_sketch_quantiles(h, s, table, [p / 1e6 for p in ppm])
    groups = {}
    for x in list(first) + list(second):
        a, st, f, svc, code = int(x["arrival_ns"]), int(x["start_ns"]), int(x["finish_ns"]), int(x["service"]), int(x["status"]) & 1
        if svc >= 5 or not a <= st <= f:
            continue
        for m, v in enumerate((st - a, f - st, f - a)):
            groups.setdefault((svc, m, 0), []).append(v)
            groups.setdefault((svc, m, 1 + code), []).append(v)
    assert groups
    for svc in range(5):
        for m in range(3):
            for c in range(3):
                v = sorted(groups.get((svc, m, c), []))
                assert int(br[svc, m, c, 0]) == len(v)
                for i, p in enumerate(ppm):
                    lo, hi = int(br[svc, m, c, 1 + 2 * i]), int(br[svc, m, c, 2 + 2 * i])
                    if v:
                        assert lo <= v[nearest_rank(len(v), p) - 1] <= hi, (svc, m, c, p)
                    else:
                        assert lo == hi == 0


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
    ok_q = _ppm_array([500_000, 990_000])

    def with_spans(h, s, n=1):
        """The entry points that take spans."""
        hh = h._h if h is not None else None
        return [lib.isim_service_sketch_host(hh, s, a, n, a),
                lib.isim_service_sketch(0, hh, s, a, n, a),
                lib.isim_service_sketch_device(hh, s, a, a, n, a, a, a, 1 << 40, None)]

    def every(h, s):
        """Every entry point that takes sub_bits; each is refused before it reads a buffer."""
        hh = h._h if h is not None else None
        return [lib.isim_service_sketch_table_words(hh, s, C.byref(out)),
                lib.isim_service_sketch_merge(hh, s, a, a),
                lib.isim_service_sketch_quantiles(hh, s, a, ok_q, 2, a)] + with_spans(h, s)

    for why, h in [("null handler", None), ("ISIM_FLAG_DYNAMIC", static), ("site graph", dag)]:
        for rc in every(h, 3) + [lib.isim_service_sketch_workspace_bytes(h._h if h is not None else None, 1, C.byref(out))]:
            _einval(rc, why)
    for rc in every(items, 8) + every(items, 0xFFFFFFFF):
        _einval(rc, "sub_bits must be 0..7")
    for rc in with_spans(items, 3, n=1 << 32) + [lib.isim_service_sketch_workspace_bytes(items._h, 1 << 32, C.byref(out))]:
        _einval(rc, "2^32 - 1")
    _einval(lib.isim_service_sketch_table_words(items._h, 3, None), "null")
    _einval(lib.isim_service_sketch_workspace_bytes(items._h, 1, None), "null")
    _einval(lib.isim_service_sketch_merge(items._h, 3, None, a), "null")
    _einval(lib.isim_service_sketch_merge(items._h, 3, a, None), "null")
    _einval(lib.isim_service_sketch_quantiles(items._h, 3, None, ok_q, 2, a), "null")
    _einval(lib.isim_service_sketch_quantiles(items._h, 3, a, ok_q, 2, None), "null")
    # the quantile list and the class count: isim_sketch_quantiles' errors
    _einval(lib.isim_service_sketch_quantiles(items._h, 3, a, None, 2, a), "null q_ppm")
    _einval(lib.isim_service_sketch_quantiles(items._h, 3, a, ok_q, 0, a), "n_q must be 1..16")
    _einval(lib.isim_service_sketch_quantiles(items._h, 3, a, _ppm_array([1_000_001]), 1, a), "above 1000000")
    big = np.zeros(isim.service_sketch_table_words(items, 3), np.uint64)
    big[2 * 6 * native.SK_BINS(3) + 5] = (1 << 40) + 1                                   # a word of the last service
    res = np.zeros(9 * native.SKQ_OUT_WORDS(2), np.uint64)
    _einval(lib.isim_service_sketch_quantiles(items._h, 3, big.ctypes.data, ok_q, 2, res.ctypes.data), "above 2^40")
    for call in (lambda *x: lib.isim_service_sketch_host(items._h, 3, *x),
                 lambda *x: lib.isim_service_sketch(0, items._h, 3, *x)):
        _einval(call(a, 1, None), "null table")
        _einval(call(None, 1, a), "null spans")
    _einval(lib.isim_service_sketch_host(items._h, 3, a, 1, a + 4), "aligned")

    need = isim.service_sketch_workspace_bytes(items, 4)

    def dev(off=a, spans=a, cap=4, info=a, table=a, ws=a, ws_bytes=1 << 30):
        return lib.isim_service_sketch_device(items._h, 3, off, spans, cap, info, table, ws, ws_bytes, None)

    for null in ("off", "info", "table", "spans"):
        _einval(dev(**{null: None}), "null")
    for mis in ("off", "info", "table", "ws"):
        _einval(dev(**{mis: a + 4}), "aligned")
    _einval(dev(spans=a + 8), "aligned")
    _einval(dev(ws_bytes=need - 1), "workspace")
    _einval(dev(ws=None), "workspace")
    with pytest.raises(isim.IsimError) as e:
        isim.DesHandler(static, 300_000).service_sketch(0, 8)
    assert e.value.code == native.EINVAL
    with pytest.raises(ValueError):
        isim.service_sketch_host(items, make_spans([]), 3, out=np.zeros(5, np.uint64))


def test_a_table_of_2_to_the_32_words_is_refused():
    """96,421 services are the fewest whose table at s = 7 reaches 2^32 words; at s = 6 theirs is accepted."""
    ns = 96_421
    assert (ns - 1) * 6 * bins_of(7) + 2 < native.SVS_MAX_WORDS <= ns * 6 * bins_of(7) + 2
    lib, h, out = native.load(), services(ns), C.c_uint64()
    a = np.zeros(8, np.uint64).ctypes.data
    for rc in [lib.isim_service_sketch_table_words(h._h, 7, C.byref(out)),
               lib.isim_service_sketch_merge(h._h, 7, a, a),
               lib.isim_service_sketch_quantiles(h._h, 7, a, _ppm_array([500_000]), 1, a),
               lib.isim_service_sketch_host(h._h, 7, a, 1, a),
               lib.isim_service_sketch(0, h._h, 7, a, 1, a),
               lib.isim_service_sketch_device(h._h, 7, a, a, 1, a, a, a, 1 << 40, None)]:
        _einval(rc, "2^32 words")
    assert isim.service_sketch_table_words(h, 6) == ns * 6 * bins_of(6) + 2
    assert isim.service_sketch_workspace_bytes(h, 0) == 256 + 3 * pad256(8 * ns)


def test_the_python_view():
    h = services(4)
    sk = isim.ServiceSketch(h, 3)
    assert sk.flat.size == 4 * 6 * 496 + 2 and not sk.flat.any() and sk.header == {"folded": 0, "refused": 0}
    assert sk.names == ["s0", "s1", "s2", "s3"] and sk.blocks.shape == (4, 3, 2, 496)
    # a hand-made table: s1 waits 100 (ten 200s), s2 waits 1000 (five 500s) and 5 (five 200s), s3 nothing
    b100, b1000 = bucket(3, 100), bucket(3, 1000)
    sk.blocks[1, native.SVQ_WAIT, 0, b100] = 10
    sk.blocks[2, native.SVQ_WAIT, 1, b1000] = 5
    sk.blocks[2, native.SVQ_WAIT, 0, 5] = 5
    sk.blocks[0, native.SVQ_WAIT, 0, 7] = 3
    for svc, n2, n5 in ((0, 3, 0), (1, 10, 0), (2, 5, 5)):
        sk.blocks[svc, native.SVQ_DURATION, 0, bucket(3, 2000 * (svc + 1))] = n2
        sk.blocks[svc, native.SVQ_DURATION, 1, bucket(3, 1 << 40)] = n5
    sk.flat[-2] = 23
    w = sk.worst("wait", 0.99, 5)
    assert [n for n, _ in w] == ["s2", "s1", "s0"]                                       # s3 has no span
    assert w[0][1] == (960, 1023) and w[1][1] == (96, 103) and w[2][1] == (7, 7)
    assert sk.worst("wait", 0.5, 1) == [("s1", (96, 103))]                               # s2's median is 5
    assert sk.worst("wait", 0.99, 5, cls="500") == [("s2", (960, 1023))]
    d = sk.quantiles((0.5,))
    assert list(d["wait"]["all"]["count"]) == [3, 10, 10, 0] and int(d["wait"]["500"]["count"][2]) == 5
    text = sk.to_text(q=(0.5, 0.99), top=2).splitlines()
    assert len(text) == 4 and text[0].startswith("service sketch of 23 spans") and "sub_bits 3" in text[0]
    assert "wait p50" in text[1] and "dur p99" in text[1]
    assert text[2].startswith("s2") and "960..1023" in text[2] and text[3].startswith("s1")
    assert isim.ServiceSketch is ServiceSketch and callable(isim.service_sketch_device)
    with pytest.raises(ValueError):
        isim.ServiceSketch(h, 3, names=["a", "b", "c"])       # one name per service
    assert isim.ServiceSketch(h, 3, names=("a", "b", "c", "d")).names == ["a", "b", "c", "d"]
