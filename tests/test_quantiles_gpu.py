"""Exact latency percentiles on the GPU (isim_latency_quantiles_device,
DESIGN.md §13) against numpy: per class (every record, the 200s, the 500s)
the count and np.sort(latency[mask])[k - 1] with k from the nearest-rank rule
restated here.  Every value must be equal as an integer."""
import json
import os

import numpy as np
import pytest

import isim
from isim import native
from isim.yamljson import yaml_to_json

from conftest import TOPOLOGIES

pytestmark = pytest.mark.gpu

# 0, 1 ppm, the Fortio report's five, 1
Q8 = (0.0, 0.000001, 0.5, 0.75, 0.9, 0.99, 0.999, 1.0)
U64 = np.uint64
BIT31 = np.uint32(1 << 31)


def rank(n, q_ppm):
    """Nearest rank, 1-based: k = max(1, ceil(q_ppm * n / 1e6)), in exact integers."""
    return max(1, -((-q_ppm * n) // 10**6))


def expect(recs, q):
    """u64[3][1 + n_q] by numpy: per class the count, then the k-th smallest latency (0s for an empty class)."""
    ppm = [round(f * 1e6) for f in q]
    is500 = (recs["status_err"] & BIT31) != 0
    out = np.zeros((3, 1 + len(q)), U64)
    for c, mask in ((native.Q_ALL, np.ones(len(recs), bool)), (native.Q_200, ~is500), (native.Q_500, is500)):
        lat = np.sort(recs["latency_ns"][mask])
        out[c, 0] = len(lat)
        for i, p in enumerate(ppm):
            if len(lat):
                out[c, 1 + i] = lat[rank(len(lat), p) - 1]
    return out


def make_recs(lat, is500=None, seed=0):
    rng = np.random.default_rng(seed)
    recs = np.zeros(len(lat), isim.REC_DTYPE)
    recs["latency_ns"] = lat
    recs["hops"] = rng.integers(0, 1 << 32, len(lat), dtype=np.uint64).astype(np.uint32)
    low = rng.integers(0, 1 << 31, len(lat), dtype=np.uint64).astype(np.uint32)
    if is500 is None:
        is500 = rng.integers(0, 2, len(lat)).astype(bool)
    recs["status_err"] = low | np.where(is500, BIT31, np.uint32(0))
    return recs


class Device:
    """Device buffers of one select: the output and a workspace, both handed over dirty."""

    def __init__(self, n_q):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.n_q = n_q
        self.ws_bytes = isim.quantiles_workspace_bytes(n_q)
        self.ws = torch.full((self.ws_bytes,), 0xA5, dtype=torch.uint8, device=self.dev)
        self.out = torch.full((isim.quantiles_out_words(n_q),), -1, dtype=torch.int64, device=self.dev)

    def upload(self, recs):
        return self.torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).copy()).to(self.dev)

    def run(self, d_records, n, q, stream=0):
        isim.latency_quantiles_device(d_records, n, q, d_out=self.out.data_ptr(), d_workspace=self.ws.data_ptr(),
                                      workspace_bytes=self.ws_bytes, stream=stream)

    def result(self):
        self.torch.cuda.synchronize()
        return self.out.cpu().numpy().view(U64).reshape(3, 1 + self.n_q)


def check(recs, q=Q8):
    d = Device(len(q))
    t = d.upload(recs)
    d.run(t.data_ptr() if len(recs) else 0, len(recs), q)
    got, want = d.result(), expect(recs, q)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    return got


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 70001])
def test_sizes_full_key_range(gpu, n):
    """Keys over the whole u64 range with 0, 2^63 and 2^64 - 1 among them, status bit 31 at random;
    70,001 records span several workgroups and a ragged tail."""
    rng = np.random.default_rng(n)
    lat = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    forced = np.array([(1 << 64) - 1, 0, 1 << 63], U64)[:n]
    lat[rng.permutation(n)[:len(forced)]] = forced
    got = check(make_recs(lat, seed=n))
    assert got[native.Q_ALL, 0] == n
    if n >= 3:
        assert got[native.Q_ALL, 1] == 0 and got[native.Q_ALL, 8] == (1 << 64) - 1


def test_constant_latency(gpu):
    """One latency in every record: a static walk without draws (64 lanes on one LDS bin)."""
    v = 4 * 250163
    got = check(make_recs(np.full(100_000, v, U64), seed=1))
    assert (got[native.Q_ALL, 1:] == v).all() and (got[native.Q_200, 1:] == v).all()
    assert (got[native.Q_500, 1:] == v).all() and got[native.Q_200, 0] + got[native.Q_500, 0] == 100_000


def peel_lanes():
    """64 lane slots for one wave: slot values 5, 4, 3 and 1 held by that many lanes, 0 by the other 51.  In
    lane order the peel (csrc/wave_peel.h) takes the 0s, the 5s and the 4s as shared keys and leaves at the 3s;
    reversed it takes the 0s and leaves at the 1, so the 3s, 4s and 5s go singly."""
    lanes = [0] * 7 + [5] * 2 + [4] + [0] * 10 + [5] * 3 + [4] * 3 + [3] * 3 + [1] + [0] * 34
    assert len(lanes) == 64 and [lanes.count(v) for v in (1, 3, 4, 5, 0)] == [1, 3, 4, 5, 51]
    return np.array(lanes, U64)


def test_peel_threshold(gpu):
    """One wave whose latencies differ in byte 1 and byte 0 with multiplicities on both sides of the peel's
    'fewer than four' break, in lane order and reversed (another leader, another break point)."""
    lat = U64(0x0A0B) + peel_lanes() * U64(0x0101)
    is500 = np.zeros(64, bool)
    for order in (slice(None), slice(None, None, -1)):
        got = check(make_recs(lat[order], is500, seed=12), q=Q8 + (51 / 64, 52 / 64, 61 / 64))
        assert got[native.Q_200].tolist() == got[native.Q_ALL].tolist() and got[native.Q_ALL, 0] == 64
    is500[peel_lanes() == 3] = True   # the class bins: 3 lanes against 61
    for order in (slice(None), slice(None, None, -1)):
        got = check(make_recs(lat[order], is500[order], seed=13))
        assert got[native.Q_500].tolist() == [3] + [0x0A0B + 3 * 0x0101] * len(Q8)


@pytest.mark.parametrize("n500", [0, 1])
def test_rank_boundary(gpu, n500):
    """500 x A then 500 x B: 500000 ppm is the 500th record (A), 500001 ppm the 501st (B)."""
    a, b = 3_000_000_123, 3_000_000_124
    rng = np.random.default_rng(5)
    lat = rng.permutation(np.array([a] * 500 + [b] * 500, U64))
    is500 = np.zeros(1000, bool)
    is500[:n500] = True
    got = check(make_recs(lat, is500, seed=2), q=(0.5, 0.500001))
    assert got[native.Q_ALL].tolist() == [1000, a, b]
    assert got[native.Q_500, 0] == n500 and got[native.Q_200, 0] == 1000 - n500


def _digit_cases():
    rng = np.random.default_rng(11)
    base = U64(0x1122334455667700)
    return {
        "byte 0 only": (base | rng.integers(0, 256, 5000, dtype=np.uint64), None),
        "byte 7 only": ((rng.integers(0, 256, 5000, dtype=np.uint64) << U64(56)) | U64(0x00AABBCCDDEEFF01), None),
        "below 256": (rng.integers(0, 256, 5000, dtype=np.uint64), None),
        "heavy duplicates": (rng.integers(0, 4, 50_000, dtype=np.uint64), None),
        "byte 3 only": (rng.integers(0, 256, 5000, dtype=np.uint64) << U64(24), None),
    }


@pytest.mark.parametrize("name", ["byte 0 only", "byte 7 only", "below 256", "heavy duplicates", "byte 3 only"])
def test_digit_structure(gpu, name):
    lat, is500 = _digit_cases()[name]
    check(make_recs(lat, is500, seed=3))


def test_empty_class(gpu):
    rng = np.random.default_rng(7)
    lat = rng.integers(0, 1 << 40, 3000, dtype=np.uint64)
    got = check(make_recs(lat, np.zeros(3000, bool), seed=4))
    assert (got[native.Q_500] == 0).all() and got[native.Q_200, 0] == 3000
    assert np.array_equal(got[native.Q_200], got[native.Q_ALL])


def test_sixteen_quantiles_and_one(gpu):
    rng = np.random.default_rng(8)
    recs = make_recs(rng.integers(0, 1 << 36, 20_000, dtype=np.uint64), seed=5)
    q16 = (0.999, 0.5, 0.5, 0.0, 1.0, 0.25, 0.999, 0.000001, 0.9, 0.75, 0.99, 0.5, 0.123456, 1.0, 0.0, 0.31)
    assert len(q16) == native.MAX_QUANTILES
    check(recs, q16)
    check(recs, (0.99,))


def test_reuse_and_offset(gpu):
    """Two selects on one workspace and one output with different data and nothing cleared in between;
    then records that start at an odd record offset inside a larger tensor."""
    rng = np.random.default_rng(9)
    first = make_recs(rng.integers(0, 1 << 64, 9000, dtype=np.uint64), seed=6)
    second = make_recs(rng.integers(0, 1 << 20, 4001, dtype=np.uint64), seed=7)
    d = Device(len(Q8))
    t1, t2 = d.upload(first), d.upload(second)
    d.run(t1.data_ptr(), len(first), Q8)
    assert np.array_equal(d.result(), expect(first, Q8))
    d.run(t2.data_ptr(), len(second), Q8)
    assert np.array_equal(d.result(), expect(second, Q8))
    d.run(t1.data_ptr() + 3 * 16, 5000, Q8)
    assert np.array_equal(d.result(), expect(first[3:5003], Q8))
    d.run(0, 0, Q8)  # no records: zeros over the previous result
    assert (d.result() == 0).all()


def _canonical_json():
    doc = json.loads(yaml_to_json(open(os.path.join(TOPOLOGIES, "canonical.yaml"), "rb").read()))
    doc.setdefault("defaults", {})["errorRate"] = 0.25
    return json.dumps(doc)


def test_end_to_end_walk(gpu):
    """serve_device writes the records, the select reads them on the same stream: the percentiles of
    Handler.serve's host records for the same trace ids."""
    import torch
    h = isim.Handler(isim.ServiceGraph.from_json(_canonical_json()), None, isim.SimParams())
    n, begin = 4096, 12345
    host, _ = h.serve(begin, n, device=0)
    dev = torch.device("cuda", 0)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    st = torch.zeros(h.stats_words, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    d = Device(len(Q8))
    h.serve_device(begin, n, rec.data_ptr(), st.data_ptr(), s)
    d.run(rec.data_ptr(), n, Q8, stream=s)
    got, want = d.result(), expect(host, Q8)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert want[native.Q_500, 0] > 0 and want[native.Q_200, 0] > 0
    # the synchronous convenience over the host records
    r = isim.latency_quantiles(host)
    assert r["all"]["count"] == n and r["500"]["count"] == int(want[native.Q_500, 0])
    w5 = expect(host, isim.DEFAULT_Q)
    for c, name in enumerate(("all", "200", "500")):
        assert [r[name]["q"][f] for f in isim.DEFAULT_Q] == w5[c, 1:].tolist()


def test_end_to_end_des(gpu):
    """The same over a DES batch (latencies include queueing): the 120-service graph under a 6 ms mean gap."""
    import torch
    from isim.generators import realistic_topology
    from isim.yamljson import obj_to_json
    j = obj_to_json(realistic_topology(120, concurrent=True, sleep_ms=(1, 5), error_rate=(0.0, 0.05)))
    h = isim.Handler(isim.ServiceGraph.from_json(j), None, isim.SimParams())
    des = isim.DesHandler(h, 6_000_000)
    n = 3000
    host, _, _ = des.serve(0, n, device=0)
    dev = torch.device("cuda", 0)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    st = torch.zeros(h.stats_words, dtype=torch.int64, device=dev)
    tab = torch.zeros(max(1, des.table_words), dtype=torch.int64, device=dev)
    wsb = des.workspace_bytes(n)
    ws = torch.empty(wsb // 8 + 1, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    d = Device(len(Q8))
    des.serve_device(0, n, rec.data_ptr(), st.data_ptr(), tab.data_ptr(), ws.data_ptr(), wsb, s)
    d.run(rec.data_ptr(), n, Q8, stream=s)
    got, want = d.result(), expect(host, Q8)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert len(np.unique(host["latency_ns"])) > n // 2  # spread latencies


def test_graph_capture(gpu):
    """One select captured on a single stream; each replay reads the records tensor as it then stands."""
    import torch
    rng = np.random.default_rng(10)
    n = 30_000
    first = make_recs(rng.integers(0, 1 << 64, n, dtype=np.uint64), seed=8)
    second = make_recs(rng.integers(0, 1 << 30, n, dtype=np.uint64), np.zeros(n, bool), seed=9)
    d = Device(len(Q8))
    t = d.upload(first)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        d.run(t.data_ptr(), n, Q8, stream=torch.cuda.current_stream().cuda_stream)
    g.replay()
    assert np.array_equal(d.result(), expect(first, Q8))
    t.copy_(d.upload(second))
    d.out.fill_(-1)
    g.replay()
    assert np.array_equal(d.result(), expect(second, Q8))
