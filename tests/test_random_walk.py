"""The seeded random graphs of tests/random_walk_graphs.py, on the CPU: the
generator's determinism, the classes its two families land in (read from
Handler(...).info, no GPU), a census of the schema corners they reach, and
the reference checking itself on this vocabulary — the pure-Python executor
against the C oracle, and the g++ build of csrc/tree_walk.h (kind 7's
per-lane code) against the C oracle — before tests/test_random_walk_gpu.py
runs the kernels on the same seeds."""
import dataclasses
import json

import pytest

import isim
import random_walk_graphs as rw
from oracle import executor_py as ex
from oracle import graph_ref as gr
from parity import oracle_params
from test_oracle import assert_python_equals_c
from test_tree_walk import checker, compare  # noqa: F401  (checker: the module's fixture)

FAMILIES = {"static": rw.static_graph, "dynamic": rw.dynamic_graph}
MODES = (isim.MODE_A, isim.MODE_B)
CASES = [(f, s) for f in FAMILIES for s in rw.SEEDS]


def info(family, seed, mode, flags=0):
    p = dataclasses.replace(rw.params(seed, mode), flags=flags)
    return isim.Handler(isim.ServiceGraph.from_json(json.dumps(FAMILIES[family](seed))), None, p).info


def test_seed_count():
    assert len(rw.SEEDS) == 48


@pytest.mark.parametrize("family", list(FAMILIES))
def test_deterministic(family):
    for seed in rw.SEEDS:
        assert json.dumps(FAMILIES[family](seed)) == json.dumps(FAMILIES[family](seed))
        assert rw.params(seed, 1) == rw.params(seed, 1)
    texts = {json.dumps(FAMILIES[family](seed)) for seed in rw.SEEDS}
    assert len(texts) > 40  # seeds name different graphs (tiny ones may coincide)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_vocabulary(family):
    """What the generator promises: 1 to 8 services, calls to higher indices,
    the family's probabilities, a bounded unrolled tree."""
    for seed in rw.SEEDS:
        doc = FAMILIES[family](seed)
        services = doc["services"]
        assert 1 <= len(services) <= 8 and doc["defaults"] == {"requestSize": 100}
        assert rw.invocations(services) <= rw.MAX_INVOCATIONS
        maybe = 0
        for i, svc in enumerate(services):
            assert svc["errorRate"] in rw.ERROR_RATES and 0 <= svc["responseSize"] <= 100000
            for step in svc["script"]:
                for c in rw.step_calls(step):
                    callee, size, prob = rw._call_of(c)
                    assert i < callee < len(services)
                    assert size is None or 0 <= size <= 5000
                    assert prob in (rw.STATIC_PROBS if family == "static" else rw.DYNAMIC_PROBS)
                    maybe += prob is not None and 1 <= prob <= 99
        assert (maybe > 0) == (family == "dynamic")


def test_static_family_classes():
    in_b = 0
    for seed in rw.SEEDS:
        assert info("static", seed, isim.MODE_A).static_walk == 1, seed
        b = info("static", seed, isim.MODE_B).static_walk
        assert b == int(seed % 2 == 0), seed  # even seeds are shaped to stay static in mode B
        in_b += b
    assert in_b >= 16 and len(rw.SEEDS) - in_b >= 16


def test_dynamic_family_classes():
    for seed in rw.SEEDS:
        for mode in MODES:
            assert info("dynamic", seed, mode).static_walk == 0, (seed, mode)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_u64_time_seeds(family):
    wide = [seed for seed in rw.SEEDS if info(family, seed, isim.MODE_A).time_bits == 64]
    assert len(wide) >= 4, wide
    for seed in rw.SEEDS:
        if seed % 8 == 3:  # the hours sleep is on a path from the entry
            assert seed in wide and rw.sleep_past_u32(FAMILIES[family](seed))


FEATURES = ("probability_0", "probability_100", "size_with_response_size", "negative_sleep_in_concurrent",
            "concurrent_only_sleeps", "empty_concurrent", "empty_script", "callee_from_several_sites",
            "always_500_mid_tree")


@pytest.mark.parametrize("family", list(FAMILIES))
def test_census(family):
    """Every corner of the schema the GPU tests are after occurs in at least 6
    seeds of the family (a condition on the generator's weights)."""
    seen = {f: [] for f in FEATURES}
    for seed in rw.SEEDS:
        for f in rw.features(FAMILIES[family](seed)):
            seen[f].append(seed)
    short = {f: s for f, s in seen.items() if len(s) < 6}
    assert not short, short
    if family == "static":  # static walks whose latency bound passes 2^32 ns
        assert sum(info("static", seed, isim.MODE_A).time_bits == 64 for seed in rw.SEEDS) >= 6


def test_params_census():
    ps = [rw.params(seed, isim.MODE_A) for seed in rw.SEEDS]
    assert len({p.seed for p in ps}) == len(ps) and any(p.seed >= 1 << 63 for p in ps)
    assert sum(p.hop_base_ns == 0 for p in ps) >= 6
    assert sum(p.hop_base_ns == 1 for p in ps) >= 6
    assert sum(10 ** 6 in (p.req_ps_per_byte, p.resp_ps_per_byte) for p in ps) >= 6
    assert sum(0 in (p.req_ps_per_byte, p.resp_ps_per_byte) for p in ps) >= 6
    assert rw.params(5, isim.MODE_B).error_mode == isim.MODE_B


@pytest.mark.parametrize("family,seed", CASES)
def test_python_vs_c_executor(family, seed):
    sg = ex.SimGraph(gr.unmarshal_service_graph(json.dumps(FAMILIES[family](seed))))
    for mode in MODES:
        assert_python_equals_c(sg, oracle_params(rw.params(seed, mode)), rw.window_begin(seed), 40)


@pytest.mark.parametrize("family,seed", CASES)
def test_tree_walk(checker, tmp_path, family, seed):  # noqa: F811
    """csrc/tree_walk.h over the program compiler's tree (every graph as a
    dynamic walk) against the C oracle.  A graph with a single sleep of 2^32 ns
    or more has no tree (include/isim.h, kernel_kind 7)."""
    doc = FAMILIES[family](seed)
    for mode in MODES:
        p = rw.params(seed, mode)
        walked = compare(checker, tmp_path, json.dumps(doc), mode, seed=p.seed, hop=p.hop_base_ns,
                         req=p.req_ps_per_byte, resp=p.resp_ps_per_byte, begin=rw.window_begin(seed), n=60)
        assert walked == (not rw.sleep_past_u32(doc)), (family, seed, mode)
