"""DES trace spans on the CPU: the Python restatement the GPU
tests check against (tests/des_spans_ref.py) is pinned to oracle/des_oracle.c;
every argument isim_serve_des_spans* refuses, found on the host before any HIP
call; the wait table's merge and size; the record's layout."""
import ctypes as C
import functools

import numpy as np
import pytest

import isim
from isim import native
from isim.des_spans import make_tap
from isim.yamljson import obj_to_json
from oracle import des as od

import des_spans_ref as ref
from test_des_gpu import DesCase
from test_des_items_gpu import CASES, MODE_B_CASES

BEGIN, N = 1000, 1500
ALL = [("a:" + k, k, isim.MODE_A) for k in sorted(CASES)] + [("b:" + k, k, isim.MODE_B) for k in sorted(MODE_B_CASES)]


@functools.lru_cache(maxsize=None)
def case_of(name, mode, mean, flags=0):
    doc = (CASES if mode == isim.MODE_A else MODE_B_CASES)[name]()
    return DesCase(doc, mean, error_mode=mode, flags=flags)


@functools.lru_cache(maxsize=None)
def invocations_of(name, mode, begin=BEGIN, n=N):
    """The executed invocations do not depend on the load: one event log per graph and batch."""
    c = case_of(name, mode, 300_000)
    return ref.invocations(c.sg, c.op, begin, n)


@functools.lru_cache(maxsize=None)
def reference(name, mode, mean, begin=BEGIN, n=N):
    """The restatement's spans of one batch, shared by every test that reads them (never modified)."""
    c = case_of(name, mode, mean)
    spans = ref.simulate(c.sg, c.op, begin, n, ref.arrivals(c.op.seed, mean, begin, n),
                         invocations_of(name, mode, begin, n))
    spans.setflags(write=False)
    return spans


@pytest.mark.parametrize("mean", [300_000, 3_000_000])
@pytest.mark.parametrize("case", ALL, ids=[c[0] for c in ALL])
def test_restatement_reproduces_the_oracle(case, mean):
    _, name, mode = case
    c = case_of(name, mode, mean)
    assert c.d.info.items == 1
    spans = reference(name, mode, mean)
    orec, _, odes = od.run(c.sg, c.op, c.sg.entry(), BEGIN, N, mean, og=c.og)
    assert np.array_equal(ref.latencies(spans), orec[:, 0])
    assert np.array_equal(np.bincount(spans["trace"].astype(np.int64) - BEGIN, minlength=N),
                          (orec[:, 1] & np.uint64(0xFFFFFFFF)).astype(np.int64))
    entry = spans[spans["hop"] == 0]
    assert np.array_equal(entry["status"] & 1, (orec[:, 1] >> np.uint64(63)).astype(np.uint32))
    t = ref.table_of(spans, len(c.sg.g.services))
    assert np.array_equal(t[:, 0], odes[:, native.DES_COUNT])
    assert np.array_equal(t[:, 1], odes[:, native.DES_SUM_WAIT])
    assert np.array_equal(t[:, 2], odes[:, native.DES_MAX_WAIT])
    assert np.array_equal(t[:, 3], odes[:, 2 * native.N_PROM] + odes[:, 2 * native.N_PROM + 1])


def test_span_record_is_64_bytes():
    assert isim.DES_SPAN_DTYPE.itemsize == 64 == C.sizeof(native.DesSpan)
    for f in ("arrival_ns", "start_ns", "finish_ns", "hop_ns", "hop", "caller_hop", "position", "slot", "service",
              "status", "replica", "reserved"):
        assert isim.DES_SPAN_DTYPE.fields[f][1] == getattr(native.DesSpan, f).offset, f
    assert C.sizeof(native.DesTap) == 88


def _handlers():
    doc = CASES["zero_hold_mix"]()
    g = isim.ServiceGraph.from_json(obj_to_json(doc))
    items = isim.Handler(g, None, isim.SimParams())
    static_doc = {"services": [{"name": "a", "isEntrypoint": True, "script": [{"sleep": "1ms"}, {"call": "b"}]},
                               {"name": "b", "script": [{"sleep": "1ms"}]}]}
    static = isim.Handler(isim.ServiceGraph.from_json(obj_to_json(static_doc)), None, isim.SimParams())
    return items, static


def test_wait_table_words_and_merge():
    h, _ = _handlers()
    lib = native.load()
    w = C.c_uint64()
    native.check(lib.isim_des_wait_table_words(h._h, C.byref(w)))
    ns = h.info.n_services
    assert w.value == (ns + 1) * native.DW_ROW_WORDS == len(isim.DesWaitTable(h).table.ravel())
    assert lib.isim_des_wait_table_words(None, C.byref(w)) == native.EINVAL
    assert lib.isim_des_wait_table_words(h._h, None) == native.EINVAL
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1 << 40, (ns + 1, native.DW_ROW_WORDS), dtype=np.uint64)
    b = rng.integers(0, 1 << 40, (ns + 1, native.DW_ROW_WORDS), dtype=np.uint64)
    want = a + b
    want[:ns, native.DW_MAX_WAIT] = np.maximum(a[:ns, native.DW_MAX_WAIT], b[:ns, native.DW_MAX_WAIT])
    ta, tb = isim.DesWaitTable(h, a.copy()), isim.DesWaitTable(h, b.copy())
    assert ta.merge(tb) is ta and np.array_equal(ta.table, want) and np.array_equal(tb.table, b)
    # the header row has no MAX word: all six add
    assert int(ta.table[ns, native.DW_MAX_WAIT]) == int(a[ns, native.DW_MAX_WAIT]) + int(b[ns, native.DW_MAX_WAIT])
    assert lib.isim_des_wait_merge(h._h, a.ctypes.data, None) == native.EINVAL
    rows = ta.rows()
    assert [r["sum_wait_ns"] for r in rows] == sorted((r["sum_wait_ns"] for r in rows), reverse=True)
    assert len(ta.to_text().splitlines()) == 2 + len(rows)


def _einval(rc, match):
    assert rc == native.EINVAL and match in native.last_error(), native.last_error()


def test_refusals_need_no_gpu():
    lib = native.load()
    items, static = _handlers()
    p = native.DesParams(300_000, 0, 0)
    buf = np.zeros(64, np.uint64)   # never dereferenced
    a = buf.ctypes.data
    assert a % 16 == 0

    def tap(**kw):
        d = dict(min_latency_ns=0, q_ppm=0, cls=0, max_traces=4, cap_spans=4, ids=a, off=a, spans=a, info=a,
                 wait_table=a)
        d.update(kw)
        return make_tap(**d)

    def dev(h, t, records=a, n=8, params=p, lp=None):
        return lib.isim_serve_des_spans_device(h._h, C.byref(params), lp, 0, n, records, a, a, a, 1 << 30,
                                               C.byref(t), None)

    def host(h, t, params=p):
        return lib.isim_serve_des_spans(h._h, 0, C.byref(params), None, 0, 8, None, None, None, C.byref(t))

    for call in (dev, host):
        _einval(call(static, tap()), "ISIM_FLAG_DYNAMIC")
        _einval(call(items, tap(max_traces=(1 << 32) + 1)), "2^32")
        _einval(call(items, tap(cap_spans=(1 << 40) + 1)), "2^40")
        _einval(call(items, tap(cls=3)), "class")
        _einval(call(items, tap(q_ppm=1_000_001)), "q_ppm")
        for null in ("ids", "off", "spans", "info"):
            _einval(call(items, tap(**{null: 0})), "null")
        t = tap()
        t.reserved[1] = 1
        _einval(call(items, t), "reserved")
        _einval(call(items, tap(), params=native.DesParams(0, 0, 0)), "mean_interarrival_ns")
    _einval(dev(items, tap(), records=None), "d_records")
    for mis in ("ids", "off", "info", "wait_table"):
        _einval(dev(items, tap(**{mis: a + 4})), "aligned")
    _einval(dev(items, tap(spans=a + 8)), "aligned")
    _einval(dev(items, tap(), records=a + 8), "aligned")
    _einval(dev(items, tap(), params=native.DesParams(300_000, 0, 7)), "reserved")
    _einval(lib.isim_serve_des_spans_device(items._h, C.byref(p), None, 0, 8, a, a, a, a, 16, C.byref(tap()), None),
            "workspace")
    _einval(lib.isim_serve_des_spans_device(items._h, None, None, 0, 8, a, a, a, a, 1 << 30, C.byref(tap()), None),
            "null")
    # a profile's errors come first, as in isim_serve_des_profile_device
    seg = (native.LoadSegment * 1)(native.LoadSegment(5, 1000))   # a last segment with a duration
    bad = native.LoadProfile(seg, 1, 0)
    _einval(dev(items, tap(), lp=C.byref(bad)), "load profile")
    # max_traces 0 and cap_spans 0 need no ids and no spans: refused only for the workspace here
    _einval(lib.isim_serve_des_spans_device(items._h, C.byref(p), None, 0, 8, a, a, a, a, 16,
                                            C.byref(tap(max_traces=0, cap_spans=0, ids=0, spans=0)), None), "workspace")
    with pytest.raises(isim.IsimError) as e:
        isim.DesHandler(static, 300_000).serve_spans(0, 8)
    assert e.value.code == native.EINVAL
