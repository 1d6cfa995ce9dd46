"""Parity of the lean mode-A draw-stream kernel (walk.hip isim_walk<4, false,
LDSC, true>; stream_walk.h walk_stream_a LEAN): the launches whose every batch
draws from the group table run a kernel with only the table form of the chunk
loop, whose group loop takes its round keys and multipliers from registers set
once per batch.  Records, stats and per-site counters are compared bit-exactly
with the C oracle: over the group counts at which the chunk loop changes (the
two-per-trip tail, the chunk boundary at 64 and 65 groups, chunks with and
without an all-zero-threshold group and an errorRate-1 record), full and
ragged batches at both high words, the ranges that must fall back to the
general kernel, both switches, and a captured launch.  The host's choice of
kernel is a pure function with a CPU truth-table test, and a launch counter
tells the GPU tests which kernel ran."""
import numpy as np
import pytest

import isim
from isim import native

from parity import Case
from oracle import executor as oc
from test_stream_group_table_gpu import _rates, _star

SEEDS = (0, 0x9E3779B97F4A7C15)
RECORDS = (1, 4, 5, 255, 256, 257, 261)  # 1, 1, 2, 64, 64, 65 and 66 groups
HI = 7 * (1 << 32) + 5
N = (1, 127, 128, 129, 293, 128 * 17 + 5)  # a wave walks 128 traces
# ... and two ranges that end just below 2^32: the invalid lanes of their one
# ragged batch lie past it, draw with the table's high word and are masked
LEAN = [(b, n) for b in (0, HI) for n in N] + [((1 << 32) - 100, 1), ((1 << 32) - 100, 100)]
FALLBACK = [((1 << 32) - 100, n) for n in N[1:]] + [((1 << 32) - 128, 256)]


def _eligible(begin, n, table=1, kind=4, mode_b=0):
    return native.load().isim_debug_lean_walk_eligible(table, kind, mode_b, begin, n)


def _case(records, seed):
    c = Case(_star(_rates(records)), None, isim.SimParams(seed=seed, error_mode=isim.MODE_A))
    assert c.handler.info.static_walk and c.handler.info.hops_upper == records
    assert c.handler.launch_info(0)["kernel_kind"] == 4
    return c


def test_eligibility_truth_table():
    top = (1 << 32) - 1
    for begin, n in LEAN:
        assert _eligible(begin, n) == 1
    for begin, n in FALLBACK:
        assert _eligible(begin, n) == 0
    assert _eligible(0, 1 << 32) == 1 and _eligible(0, (1 << 32) + 1) == 0
    assert _eligible(top, 1) == 1 and _eligible(top, 2) == 0
    assert _eligible(1 << 32, 1 << 31) == 1
    assert _eligible((1 << 32) - 100, 100) == 1 and _eligible((1 << 32) - 100, 101) == 0
    assert _eligible((1 << 64) - 4, 4) == 1 and _eligible((1 << 64) - 4, 5) == 0  # wraps past 2^64
    assert _eligible(0, 0) == 0
    # no table, another kernel kind, mode B
    assert _eligible(0, 128, table=0) == 0
    for kind in (0, 1, 2, 3, 5, 6, 7, 8):
        assert _eligible(0, 128, kind=kind) == 0
    assert _eligible(0, 128, mode_b=1) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("switch", [None, "ISIM_NO_LEAN_WALK", "ISIM_NO_GROUP_TABLE"])
@pytest.mark.parametrize("records", RECORDS)
def test_star(gpu, records, switch, monkeypatch):
    # the switches are read when the handler prepares the device
    if switch:
        monkeypatch.setenv(switch, "1")
    lib = native.load()
    for seed in SEEDS:
        c = _case(records, seed)
        for ranges, lean in ((LEAN, switch is None), (FALLBACK, False)):
            for begin, n in ranges:
                before = lib.isim_debug_lean_walk_launches()
                c.compare(begin, n)
                # one launch each: the lean kernel ran it, or the general one
                assert lib.isim_debug_lean_walk_launches() - before == (1 if lean else 0), (begin, n)


@pytest.mark.gpu
def test_graph_capture(gpu):
    # one captured serve_device on the lean path (the table's build kernel, the
    # lean walk and the counter fold), replayed twice, against two eager calls
    import torch
    dev = torch.device("cuda", 0)
    c = _case(261, SEEDS[1])
    begin, n = HI, 293
    assert _eligible(begin, n) == 1
    before = native.load().isim_debug_lean_walk_launches()
    c.gpu(begin, n)  # the first call prepares the device
    assert native.load().isim_debug_lean_walk_launches() == before + 1
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
    packed = got["hops"].astype(np.uint64) | (got["status_err"].astype(np.uint64) << np.uint64(32))
    assert np.array_equal(packed, orec[:, 1])
    o = oc.split_stats(ost, len(c.sg.g.services), len(c.sg.sites))
    f = c.handler.fold(st_g.cpu().numpy().view(np.uint64))
    assert f["n_500"] == 2 * o["n_500"] and f["n_traces"] == 2 * n
    assert np.array_equal(np.asarray(f["svc_errs"], np.uint64), 2 * np.asarray(o["svc_errs"], np.uint64))
