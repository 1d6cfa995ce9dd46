"""Per-window exact latency percentiles on the GPU:
isim_timeline_quantiles* against numpy over rows computed with Python
integers, `np.sort(lat[mask])[k - 1]` with k from a restatement of the
nearest-rank rule; against the timeline table and the whole-batch select; with
dirty buffers under graph capture; and through DesHandler on an overloaded
tree.  Every comparison is equality of integers."""
import json
import os
import re

import numpy as np
import pytest

import isim
from isim import native
from isim.yamljson import yaml_to_json

from conftest import ROOT, TOPOLOGIES
from test_timeline_gpu import WINDOWS, arrivals_np, make_case, make_recs, peel_case, rows_of

pytestmark = pytest.mark.gpu

U64 = np.uint64
MAXU = (1 << 64) - 1
BIT31 = np.uint32(1 << 31)
Q7 = isim.DEFAULT_Q + (0.0, 1.0)   # the five defaults plus 0 and 10^6 ppm
KSTAGE = 3584                      # latencies of a row the select keeps in LDS (csrc/segmented_select.h kStage)


def nearest_rank(n, ppm):
    """max(1, ceil(ppm * n / 10^6)) in Python integers."""
    return max(1, -(-ppm * n // 1_000_000))


def expect(arr, recs, t0, window, n_windows, q):
    """The table u64[n_windows + 2][3][1 + n_q], flat."""
    ppm = isim.quantiles.q_to_ppm(q)
    arr = np.asarray(arr, U64)
    lat = recs["latency_ns"].astype(U64)
    c = arr + lat
    c = np.where(c < arr, U64(MAXU), c)  # saturates
    rc = rows_of(c, t0, window, n_windows) if len(arr) else np.zeros(0, np.int64)
    is500 = (recs["status_err"] & BIT31) != 0
    out = np.zeros((n_windows + 2, 3, 1 + len(ppm)), U64)
    order = np.argsort(rc, kind="stable")
    rows, first = np.unique(rc[order], return_index=True)
    for r, a, b in zip(rows, first, list(first[1:]) + [len(order)]):
        idx = order[a:b]
        for cls, mask in ((native.Q_ALL, np.ones(len(idx), bool)), (native.Q_200, ~is500[idx]),
                          (native.Q_500, is500[idx])):
            v = np.sort(lat[idx][mask])
            if len(v):
                out[r, cls, 0] = len(v)
                out[r, cls, 1:] = [v[nearest_rank(len(v), p) - 1] for p in ppm]
    return out.reshape(-1)


def check(arr, recs, t0, window, n_windows, q=Q7, note=None):
    got = isim.timeline_quantiles_table(arr, recs, window, n_windows, t0, q)
    want = expect(arr, recs, t0, window, n_windows, q)
    bad = np.argwhere(got != want)
    w = 3 * (1 + len(q))
    assert bad.size == 0, (note, [(int(i) // w, int(i) % w // (1 + len(q)), int(i) % (1 + len(q)), int(got[i]),
                                   int(want[i])) for i in bad[:4, 0]])
    return got.reshape(n_windows + 2, 3, 1 + len(q))


def test_restatement_and_stage_constant():
    for n, ppm in ((1, 0), (1, 10**6), (1000, 500_000), (1000, 500_001), (3, 999_000), (70_001, 990_000), (1 << 32, 1)):
        assert nearest_rank(n, ppm) == isim.quantile_rank(n, ppm)
    src = open(os.path.join(ROOT, "istio-isotope_amd", "csrc", "segmented_select.h")).read()
    assert int(re.search(r"constexpr uint32_t kStage = (\d+);", src).group(1)) == KSTAGE
    abi = open(os.path.join(ROOT, "include", "isim.h")).read()
    assert int(re.search(r"#define ISIM_SVQ_STAGE (\d+)", abi).group(1)) == KSTAGE


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 70_001])
@pytest.mark.parametrize("window,n_windows", WINDOWS)
def test_against_numpy(gpu, n, window, n_windows):
    for t0_mode in (0, 1):
        arr, recs, t0 = make_case(n, window, n_windows, t0_mode, seed=n * 7 + n_windows + t0_mode)
        for permuted in (False, True):
            if permuted:
                p = np.random.default_rng(n).permutation(n)
                arr, recs = arr[p], recs[p]
            t = check(arr, recs, t0, window, n_windows, note=(t0_mode, permuted))
            assert int(t[:, native.Q_ALL, 0].sum()) == n == int(t[:, native.Q_200, 0].sum() + t[:, native.Q_500, 0].sum())


def _rows_case(sizes, window, seed, lat_hi=None):
    """Row 1 + w holds exactly sizes[w] records: arrivals at the window's start, latencies below the window."""
    rng = np.random.default_rng(seed)
    arr = np.concatenate([np.full(s, w * window, U64) for w, s in enumerate(sizes)] + [np.zeros(0, U64)])
    lat = rng.integers(0, lat_hi or window, len(arr), dtype=np.uint64)
    p = rng.permutation(len(arr))
    return arr[p], make_recs(lat, seed + 1)[p]


def test_staging_edge(gpu):
    """Rows of kStage - 1, kStage and kStage + 1 records (the last re-reads its
    segment per digit), with short rows around them; one row holding all of 70,001."""
    sizes = [5, KSTAGE - 1, 0, KSTAGE, 1, KSTAGE + 1, 64]
    arr, recs = _rows_case(sizes, 10**6, 11)
    t = check(arr, recs, 0, 10**6, len(sizes))
    assert t[1:-1, native.Q_ALL, 0].tolist() == sizes
    # single-class rows at the edge: every record a 200
    recs["status_err"] &= ~BIT31
    t = check(arr, recs, 0, 10**6, len(sizes))
    assert t[1:-1, native.Q_200, 0].tolist() == sizes and not t[:, native.Q_500].any()
    arr, recs = _rows_case([70_001], 1 << 40, 12)
    t = check(arr, recs, 0, 1 << 40, 1)
    assert int(t[1, native.Q_ALL, 0]) == 70_001
    # and in "after": windows that end before the first completion
    arr, recs = _rows_case([70_001], 1 << 40, 13, lat_hi=1 << 39)
    t = check(arr + U64(1 << 41), recs, 0, 1, 65536)
    assert int(t[-1, native.Q_ALL, 0]) == 70_001


@pytest.mark.parametrize("n", [64, 320, 5000])
def test_all_latencies_equal(gpu, n):
    """64 lanes on one bin in every digit pass; also all zero (no digit pass) and all 2^64 - 1."""
    for value in (8_000_000, 0, MAXU, 1 << 63):
        recs = make_recs(np.full(n, value, U64), n)
        t = check(np.full(n, 123_456_789, U64), recs, 0, 10**6, 200, note=value)
        row = 132 if value == 8_000_000 else 124 if value == 0 else 201
        assert int(t[row, native.Q_ALL, 0]) == n and (t[row, native.Q_ALL, 1:] == U64(value)).all()


def test_peel_threshold(gpu):
    """test_timeline_gpu.peel_case: one wave whose latencies have multiplicities on both sides of the peel's
    'fewer than four' break (csrc/wave_peel.h), in lane order and reversed.  Every completion in one row (the
    select's bins; with the 3 lanes of one value as 500s also the (row, code) counters and cursors), then
    in rows with those multiplicities (counters and cursors)."""
    q = Q7 + (51 / 64, 52 / 64, 61 / 64)
    for reverse in (False, True):
        arr, recs = peel_case(reverse)
        t = check(arr, recs, 0, 10**6, 8, q, note=reverse)
        assert t[9, native.Q_200, 0] == 64
        recs["status_err"][recs["latency_ns"] == 14_500_000] |= BIT31
        t = check(arr, recs, 0, 10**6, 8, q, note=reverse)
        assert t[9, :, 0].tolist() == [64, 61, 3]
        arr[:] = 5
        t = check(arr, recs, 0, 10**6, 30, q, note=reverse)
        assert sorted(t[:, native.Q_ALL, 0].tolist())[-5:] == [1, 3, 4, 5, 51]


@pytest.mark.parametrize("byte", range(8))
def test_one_byte_differs(gpu, byte):
    """Latencies equal but for one byte: every other digit pass sees one bin."""
    rng = np.random.default_rng(byte)
    for n in (500, KSTAGE + 500):
        base = 0x5A3C_9617_E2D4_0B81 & ~(0xFF << (8 * byte))
        lat = U64(base) | (rng.integers(0, 256, n, dtype=np.uint64) << U64(8 * byte))
        check(np.zeros(n, U64), make_recs(lat, byte + 10), 0, MAXU, 1, note=n)


def test_duplicates_at_a_rank_boundary(gpu):
    """An even count, half A and half B > A: 500,000 ppm is the last A, 500,001 ppm the first B."""
    q = (0.5, 0.500001, 0.499999, 0.0, 1.0)
    for n, a, b in ((1000, 7_000_000, 7_000_001), (2 * KSTAGE + 2, 1 << 40, (1 << 40) + (1 << 32)), (64, 0, MAXU - 1)):
        lat = np.concatenate([np.full(n // 2, a, U64), np.full(n // 2, b, U64)])
        recs = make_recs(lat, n)
        recs["status_err"] &= ~BIT31
        p = np.random.default_rng(n).permutation(n)
        t = check(np.zeros(n, U64), recs[p], 0, MAXU, 1, q)
        assert t[1, native.Q_200].tolist() == [n, a, b, a, a, b] == t[1, native.Q_ALL].tolist()


def test_classes_and_empty_rows(gpu):
    """Row 1 only 500s, row 3 only 200s, row 6 one record, rows 2, 4, 5, 7 empty, nothing before or after."""
    window = 1000
    rng = np.random.default_rng(5)
    arr = np.concatenate([np.full(300, 0, U64), np.full(200, 2 * window, U64), np.full(1, 5 * window, U64)])
    recs = make_recs(rng.integers(0, window, len(arr), dtype=np.uint64), 6)
    recs["status_err"][:300] |= BIT31
    recs["status_err"][300:] &= ~BIT31
    t = check(arr, recs, 0, window, 7)
    assert t[:, native.Q_ALL, 0].tolist() == [0, 300, 0, 200, 0, 0, 1, 0, 0]
    assert t[:, native.Q_500, 0].tolist() == [0, 300, 0, 0, 0, 0, 0, 0, 0]
    assert t[:, native.Q_200, 0].tolist() == [0, 0, 0, 200, 0, 0, 1, 0, 0]
    assert not t[[0, 2, 4, 5, 7, 8]].any() and not t[1, native.Q_200].any() and not t[3, native.Q_500].any()
    assert (t[6, native.Q_200, 1:] == recs["latency_ns"][-1]).all()


def test_sixteen_unsorted_quantiles(gpu):
    q = (0.999, 0.5, 0.0, 1.0, 0.5, 0.25, 0.999999, 0.000001, 0.9, 0.99, 0.75, 0.9, 0.1, 1.0, 0.333333, 0.5)
    assert len(q) == native.MAX_QUANTILES
    arr, recs, t0 = make_case(20_000, 10**6, 2, 1, seed=77)
    check(arr, recs, t0, 10**6, 2, q)
    arr, recs = _rows_case([KSTAGE + 77, 3, 900], 10**6, 78, lat_hi=1 << 20)
    check(arr, recs, 0, 10**6, 3, q)
    check(arr, recs, 0, 10**6, 3, (0.5,))


def test_against_the_timeline_table(gpu):
    """Counts are the timeline's DONE words, the 10^6-ppm value its MAX_LAT."""
    for window, n_windows in ((7, 37), (10**6, 300), (1 << 40, 65536)):
        arr, recs, t0 = make_case(9000, window, n_windows, 1, seed=n_windows)
        tq = isim.timeline_quantiles_table(arr, recs, window, n_windows, t0, (0.5, 1.0)).reshape(n_windows + 2, 3, 3)
        tl = isim.timeline_table(arr, recs, window, n_windows, t0).reshape(n_windows + 2, native.TL_ROW_WORDS)
        for code, cls in ((0, native.Q_200), (1, native.Q_500)):
            assert np.array_equal(tq[:, cls, 0], tl[:, native.TL_DONE + code])
            assert np.array_equal(tq[:, cls, 2], tl[:, native.TL_MAX_LAT + code])
        assert np.array_equal(tq[:, native.Q_ALL, 0], tl[:, native.TL_DONE] + tl[:, native.TL_DONE + 1])
        assert np.array_equal(tq[:, native.Q_ALL, 2], np.maximum(tl[:, native.TL_MAX_LAT], tl[:, native.TL_MAX_LAT + 1]))


def test_against_the_whole_batch_select(gpu):
    """One window that takes every record gives isim_latency_quantiles of the same records."""
    rng = np.random.default_rng(9)
    n = 50_000
    lat = rng.integers(0, 1 << 62, n, dtype=np.uint64) >> rng.integers(0, 60, n, dtype=np.uint64)
    recs = make_recs(lat, 10)
    arr = rng.integers(0, 1 << 61, n, dtype=np.uint64)
    t = isim.timeline_quantiles(arr, recs, MAXU, 1, 0, Q7)
    whole = isim.latency_quantiles(recs, Q7)
    for c, name in enumerate(("all", "200", "500")):
        assert int(t["count"][c, 0]) == whole[name]["count"] > 0
        assert [int(x) for x in t["latency_ns"][c, :, 0]] == [whole[name]["q"][f] for f in Q7]
    assert not t["before"]["count"].any() and not t["after"]["count"].any() and t["q"] == Q7


def _upload(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(torch.device("cuda", 0))


def test_dirty_buffers_and_capture(gpu):
    """Workspace and out filled with 0xA5; arrivals and the timeline quantiles
    captured as one chain, with nothing run before the capture.  The table is
    written, not accumulated: one replay and three give the same table."""
    import torch
    doc = {"services": [{"name": "a", "isEntrypoint": True, "script": [{"sleep": "1ms"}]}]}
    handler = isim.Handler(isim.ServiceGraph.from_json(json.dumps(doc)), None, isim.SimParams(seed=0x5EED0123456789AB))
    n, mean, begin, window, n_windows = 20_000, 50_000, 99, 250_000_000, 6   # about 5000 records per row, 4 rows
    dev = torch.device("cuda", 0)
    awsb = isim.des_arrivals_workspace_bytes(n)
    aws = torch.full((awsb,), 0xA5, dtype=torch.uint8, device=dev)
    wsb = isim.timeline_quantiles_workspace_bytes(n, n_windows, len(Q7))
    ws = torch.full((wsb,), 0xA5, dtype=torch.uint8, device=dev)
    words = isim.timeline_quantiles_out_words(n_windows, len(Q7))
    out = torch.full((words * 8,), 0xA5, dtype=torch.uint8, device=dev)
    d_arr = torch.full((n,), -1, dtype=torch.int64, device=dev)
    want_arr = arrivals_np(handler.params.seed, mean, begin, n)
    lat = np.random.default_rng(4).integers(0, 4 * 10**7, n, dtype=np.uint64)
    lat[::7] = 0
    recs = make_recs(lat, 6)
    d_rec = _upload(torch, recs)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        s = torch.cuda.current_stream().cuda_stream
        isim.des_arrivals_device(handler, mean, begin, n, d_arrivals=d_arr.data_ptr(), d_workspace=aws.data_ptr(),
                                 workspace_bytes=awsb, stream=s)
        isim.timeline_quantiles_device(d_arr.data_ptr(), d_rec.data_ptr(), n, window, n_windows, 0, Q7,
                                       d_out=out.data_ptr(), d_workspace=ws.data_ptr(), workspace_bytes=wsb, stream=s)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(d_arr.cpu().numpy().view(U64), want_arr)
    want = expect(want_arr, recs, 0, window, n_windows, Q7)
    assert np.array_equal(out.cpu().numpy().view(U64), want)
    assert want.reshape(-1, 3, 1 + len(Q7))[:, 0, 0].max() > KSTAGE   # a row past the staging
    ws.fill_(0x5A)
    out.fill_(0x5A)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(U64), want)
    # an empty batch through the device entry: every word of a dirty table becomes 0
    out.fill_(0xA5)
    isim.timeline_quantiles_device(0, 0, 0, window, n_windows, 0, Q7, d_out=out.data_ptr(), d_workspace=ws.data_ptr(),
                                   workspace_bytes=wsb, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()


def test_end_to_end_des(gpu):
    """DesHandler.timeline_quantiles on the committed 13-service tree with a
    2 ms sleep in every service, at a 1 ms mean gap (overloaded: the queue
    grows, and the p99 of what completes with it)."""
    doc = json.loads(yaml_to_json(open(os.path.join(TOPOLOGIES, "tree-13-services.yaml"), "rb").read()))
    for s in doc["services"]:
        s["script"] = [{"sleep": "2ms"}] + (s.get("script") or [])
        s["errorRate"] = 0.05
    h = isim.Handler(isim.ServiceGraph.from_json(json.dumps(doc)), None, isim.SimParams())
    d = isim.DesHandler(h, 1_000_000)
    n, begin, window, n_windows = 6000, 17, 250_000_000, 20
    tq = d.timeline_quantiles(begin, n, window, n_windows)
    recs, _, _ = d.serve(begin, n)
    arr = d.arrivals(begin, n)
    want = isim.decode_timeline_quantiles(expect(arr, recs, 0, window, n_windows, isim.DEFAULT_Q), n_windows, 0, window,
                                          len(isim.DEFAULT_Q))
    assert tq["q"] == isim.DEFAULT_Q
    for k in ("count", "latency_ns"):
        assert np.array_equal(tq[k], want[k]), k
        assert np.array_equal(tq["after"][k], want["after"][k]) and not tq["before"][k].any(), k
    assert int(tq["count"][native.Q_ALL].sum() + tq["after"]["count"][native.Q_ALL]) == n
    assert tq["count"][native.Q_500].sum() > 0
    p99 = tq["latency_ns"][native.Q_200, isim.DEFAULT_Q.index(0.99)]
    assert 0 < p99[1] <= p99[n_windows // 2] <= p99[-1]
