"""GPU parity of the draw-stream walks' per-launch group table (kernel_abi.h
GroupEnt, walk.hip isim_group_table): rounds 1-2 of the wave-uniform Philox
counter words and the group's record tests, computed once per launch and read
by every wave instead of being derived per wave and group.  Any wrong table
word changes a draw, so records, stats and per-site counters are compared
bit-exactly with the C oracle, for every draw-stream kind, over the group
counts, trace counts, trace ids and seeds at which the table's use changes:
the chunk boundary and the two-per-trip loop's tail, full and ragged batches,
a non-zero high word, batches that straddle 2^32 (no table), a launch whose
second batch has another high word than the table's, and the launches without
a table."""
import json

import numpy as np
import pytest

import isim

from parity import Case
from oracle import executor as oc

pytestmark = pytest.mark.gpu

# (error mode, flags, kernel kind) of a static walk
VARIANTS = {
    "A": (isim.MODE_A, 0, 4),
    "B-mark": (isim.MODE_B, 0, 8),
    "B-closelist": (isim.MODE_B, isim.native.FLAG_CLOSE_LIST, 6),
    "B-bitstack": (isim.MODE_B, isim.native.FLAG_BIT_STACK, 5),
}
SEEDS = (0, 0x9E3779B97F4A7C15)  # zero; both halves non-zero
RECORDS = (1, 4, 5, 255, 256, 257, 261)  # 1, 1, 2, 64, 64, 65 and 66 groups
TRACES = (1, 127, 128, 129, 293)  # a wave walks 128 traces: ragged, full, full + ragged
HI = 7 * (1 << 32) + 5
# (trace_begin, n): every trace count at t_hi 0, at a non-zero t_hi, and with
# the first batch straddling 2^32; then two full batches of which the second
# has another t_hi than the launch's table
RANGES = [(b, n) for b in (0, HI, (1 << 32) - 100) for n in TRACES] + [((1 << 32) - 128, 256)]


def _rates(records):
    """Error rates of the records 1..records-1 of a star; from 41 records on,
    group 2 (records 8-11) never errs (an all-zero-threshold group) and record
    18 always does (an errorRate-1 record mid-stream)."""
    rates = [0.005 + 0.01 * (i % 5) for i in range(records - 1)]
    if records >= 41:
        for r in range(8, 12):
            rates[r - 1] = 0
        rates[18 - 1] = 1.0
    return rates


def _star(rates):
    """Entry calling len(rates) leaves in one concurrent step (a static walk
    in both modes): stream record r (1-based) is leaf r - 1."""
    svcs = [{"name": "e", "isEntrypoint": True, "errorRate": 0.01,
             "script": [[{"call": f"l{i}"} for i in range(len(rates))]] if rates else []}]
    svcs += [{"name": f"l{i}", "errorRate": r} for i, r in enumerate(rates)]
    return json.dumps({"services": svcs})


def _chain(n, fan, rate=0.02, leaf_rate=0.03):
    """c0 -> c1 -> ... -> c(n-1), each link also calling `fan` leaves after its
    child in one concurrent step: n (1 + fan) - fan records, call depth n."""
    svcs = []
    for i in range(n):
        calls = [[{"call": f"c{i + 1}"}] + [{"call": f"l{i}-{j}"} for j in range(fan)]] if i + 1 < n else []
        svcs.append({"name": f"c{i}", "script": [{"sleep": "1us"}] + calls, "errorRate": rate})
        if i + 1 < n:
            svcs += [{"name": f"l{i}-{j}", "errorRate": leaf_rate} for j in range(fan)]
    svcs[0]["isEntrypoint"] = True
    return json.dumps({"services": svcs})


def _case(j, variant, seed, kind=None):
    mode, flags, k = VARIANTS[variant]
    c = Case(j, None, isim.SimParams(seed=seed, error_mode=mode, flags=flags))
    assert c.handler.info.static_walk
    assert c.handler.launch_info(0)["kernel_kind"] == (k if kind is None else kind)
    return c


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("records", RECORDS)
def test_star(gpu, records, variant):
    j = _star(_rates(records))
    for seed in SEEDS:
        c = _case(j, variant, seed)
        assert c.handler.info.hops_upper == records
        for begin, n in RANGES:
            c.compare(begin, n)


@pytest.mark.parametrize("variant", ["A", "B-mark", "B-closelist", "B-bitstack"])
def test_deep_chain(gpu, variant):
    # 97 records (25 groups, an odd count) at call depth 33: deeper than the
    # bit stack, so its flag runs kind 4 in mode B (the wave-mask stack)
    j = _chain(33, 2)
    for seed in SEEDS:
        c = _case(j, variant, seed, kind=4 if variant == "B-bitstack" else None)
        assert c.handler.info.hops_upper == 97 and c.handler.info.max_depth > 32
        for begin, n in RANGES:
            c.compare(begin, n)


@pytest.mark.parametrize("variant", ["A", "B-mark", "B-closelist", "B-bitstack", "B-deep"])
def test_no_table(gpu, variant, monkeypatch):
    # the launches of a stream past the table's size cap pass no table and
    # keep the scalar rounds in the kernel: here by the library's test switch,
    # read when the handler prepares the device
    monkeypatch.setenv("ISIM_NO_GROUP_TABLE", "1")
    if variant == "B-deep":
        c = _case(_chain(33, 2), "B-bitstack", SEEDS[1], kind=4)
    else:
        c = _case(_star(_rates(261)), variant, SEEDS[1])
    for begin, n in [(0, 293), (HI, 129), ((1 << 32) - 100, 293), ((1 << 32) - 128, 256)]:
        c.compare(begin, n)


def test_graph_capture(gpu):
    # one captured serve_device of kind 4 (the table's build kernel, the walk
    # and the counter fold), replayed twice, against two eager calls
    import torch
    dev = torch.device("cuda", 0)
    c = _case(_star(_rates(261)), "A", SEEDS[1])
    begin, n = HI, 293
    c.gpu(begin, n)  # the first call prepares the device
    words = c.handler.stats_words
    rec_e = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    st_e = torch.zeros(words, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(2):
        c.handler.serve_device(begin, n, rec_e.data_ptr(), st_e.data_ptr(), s)
    torch.cuda.synchronize()
    rec_g = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    st_g = torch.zeros(words, dtype=torch.int64, device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        c.handler.serve_device(begin, n, rec_g.data_ptr(), st_g.data_ptr(), torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(rec_g.cpu().numpy(), rec_e.cpu().numpy())
    assert np.array_equal(st_g.cpu().numpy(), st_e.cpu().numpy())
    # and both are the oracle's: the records of one call, the statistics of two
    orec, ost = c.cpu(begin, n)
    got = rec_g.cpu().numpy().view(isim.REC_DTYPE)
    assert np.array_equal(got["latency_ns"], orec[:, 0])
    o = oc.split_stats(ost, len(c.sg.g.services), len(c.sg.sites))
    f = c.handler.fold(st_g.cpu().numpy().view(np.uint64))
    assert f["n_500"] == 2 * o["n_500"] and f["n_traces"] == 2 * n
    assert np.array_equal(np.asarray(f["svc_errs"], np.uint64), 2 * np.asarray(o["svc_errs"], np.uint64))
