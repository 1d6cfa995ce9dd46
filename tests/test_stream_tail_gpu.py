"""GPU parity of the draw-stream walks' per-record tail (stream_walk.h): the
per-site 500 counts collected per chunk instead of per record, the per-trace
error count, the errorRate-1 and all-zero-threshold groups, ragged and
2^32-straddling batches.  Records and stats bit-exact against the C oracle,
for the mode-A walk (kind 4) and the mode-B walks by marking (kind 8), close
list (kind 6) and bit stack (kind 5)."""
import json

import numpy as np
import pytest

import isim

from parity import Case, assert_stats_equal
from oracle import executor as oc

pytestmark = pytest.mark.gpu

# (error mode, flags) -> kernel kind of a static walk
VARIANTS = {
    "A": (isim.MODE_A, 0, 4),
    "A-closelist": (isim.MODE_A, isim.native.FLAG_CLOSE_LIST, 4),
    "A-bitstack": (isim.MODE_A, isim.native.FLAG_BIT_STACK, 4),
    "B-mark": (isim.MODE_B, 0, 8),
    "B-closelist": (isim.MODE_B, isim.native.FLAG_CLOSE_LIST, 6),
    "B-bitstack": (isim.MODE_B, isim.native.FLAG_BIT_STACK, 5),
}


def _star(rates):
    """Entry calling len(rates) leaves in one concurrent step (no mode-B
    abort between them: a static walk in both modes): stream record r
    (1-based) is leaf r - 1, so error rates are placed by record position."""
    svcs = [{"name": "e", "isEntrypoint": True, "errorRate": 0.01,
             "script": [[{"call": f"l{i}"} for i in range(len(rates))]] if rates else []}]
    svcs += [{"name": f"l{i}", "errorRate": r} for i, r in enumerate(rates)]
    return json.dumps({"services": svcs})


def _chain(n, fan, rate=0.02, leaf_rate=0.03):
    """c0 -> c1 -> ... -> c(n-1), each link also calling `fan` leaves after its
    child, in one concurrent step (subtrees that close inside, at and across chunk boundaries):
    n (1 + fan) - fan records."""
    svcs = []
    for i in range(n):
        calls = [[{"call": f"c{i + 1}"}] + [{"call": f"l{i}-{j}"} for j in range(fan)]] if i + 1 < n else []
        svcs.append({"name": f"c{i}", "script": [{"sleep": "1us"}] + calls, "errorRate": rate})
        if i + 1 < n:
            svcs += [{"name": f"l{i}-{j}", "errorRate": leaf_rate} for j in range(fan)]
    svcs[0]["isEntrypoint"] = True
    return json.dumps({"services": svcs})


def _case(j, variant):
    mode, flags, kind = VARIANTS[variant]
    c = Case(j, None, isim.SimParams(error_mode=mode, flags=flags))
    assert c.handler.info.static_walk
    if kind == 5 and c.handler.info.max_depth > 32:
        kind = 4  # deeper than the bit stack: the wave-mask stack
    assert c.handler.launch_info(0)["kernel_kind"] == kind
    return c


# 300 traces: more than one wave (128 traces each), the last one ragged
N = 300


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("records", [63, 64, 65, 255, 256, 257, 261])
def test_chunk_boundary_star(gpu, records, variant):
    # a chunk boundary (32 records: close list; 64: the marks' counts;
    # 256 = 64 groups: mode A's counts) inside the stream and at its end
    rates = [0.005 + 0.01 * (i % 5) for i in range(records - 1)]
    c = _case(_star(rates), variant)
    assert c.handler.info.hops_upper == records
    c.compare(0, N)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("n,fan", [(16, 3), (22, 2), (33, 1), (52, 4), (64, 4)])
def test_chunk_boundary_chain(gpu, n, fan, variant):
    # 61, 64, 65, 256 and 316 records with nested subtrees closing across the boundaries
    c = _case(_chain(n, fan), variant)
    assert c.handler.info.hops_upper == n * (1 + fan) - fan
    c.compare(7, N)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("leaves", [0, 2, 3])
def test_single_group(gpu, leaves, variant):
    # n_groups == 1: 1, 3 (one padding record) and 4 records
    c = _case(_star([0.3] * leaves), variant)
    assert c.handler.info.hops_upper == 1 + leaves
    c.compare(0, N)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("pos", [30, 31, 63, 64, 255])
def test_always_record(gpu, pos, variant):
    # one errorRate-1 service at record `pos`: mid-chunk, and the last and
    # first record of a chunk
    rates = [0.02] * 259
    rates[pos - 1] = 1.0
    _case(_star(rates), variant).compare(0, N)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_zero_threshold_groups(gpu, variant):
    # records 6..21 never err: groups 2..4 are all-zero-threshold groups
    # (their draws are skipped), groups 1 and 5 are partly zero
    rates = [0.05] * 40
    for r in range(6, 22):
        rates[r - 1] = 0
    _case(_star(rates), variant).compare(0, N)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("pos", [31, 63, 255])
def test_error_on_last_record_of_chunk(gpu, pos, variant):
    # the only erring records: the last of a chunk and the first of the stream's last group
    rates = [0] * 259
    rates[pos - 1] = 0.5
    rates[256] = 0.5
    _case(_star(rates), variant).compare(0, N)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_trace_ids_straddle_2_32(gpu, variant):
    # t_hi differs inside the first wave and between the two
    c = _case(_chain(22, 2), variant)
    c.compare((1 << 32) - 64, 256)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_ragged_batch_straddles_2_32(gpu, variant):
    # one wave, 100 of its 128 trace slots valid, t_hi differing inside it:
    # the ragged walk together with the per-trace (not lockstep) draws
    c = _case(_chain(22, 2), variant)
    c.compare((1 << 32) - 30, 100)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_high_error_rate(gpu, variant):
    # 50 %: many lanes err at one record, in both traces of a lane, and a lane
    # errs several times within a group; the per-trace error count is the
    # records' err field, the per-site counts are in the stats
    for j in (_star([0.5] * 70), _chain(9, 3, rate=0.5, leaf_rate=0.5)):
        c = _case(j, variant)
        recs, _ = c.compare(3, N)
        assert int((recs["status_err"] & 0x7FFFFFFF).max()) >= 8


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_two_launches_one_stats_buffer(gpu, variant):
    # the per-chunk accumulators start clean in every launch: two launches
    # into one device stats buffer sum to the oracle's statistics of both ranges
    import torch
    c = _case(_chain(22, 2, rate=0.1, leaf_rate=0.2), variant)
    dev = torch.device("cuda", 0)
    st = torch.zeros(c.handler.stats_words, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    c.handler.serve_device(0, N, 0, st.data_ptr(), s)
    c.handler.serve_device(N, 1000, 0, st.data_ptr(), s)
    torch.cuda.synchronize()
    got = st.cpu().numpy().view(np.uint64)
    _, ost = c.cpu(0, N + 1000, records=False)
    assert_stats_equal(c.handler.fold(got), oc.split_stats(ost, len(c.sg.g.services), len(c.sg.sites)))
