"""The seeded random DES cases of tests/random_des_graphs.py, on the CPU: the
classes isim.DesHandler puts them in and the refusals, a census of the schema
corners and of the contention they reach, and the references checking each
other on this vocabulary — the Python restatement of the DES
(tests/des_spans_ref.py) against oracle/des_oracle.c on every accepted case,
level-engine graphs included, and the pooled restatement
(tests/des_workers_ref.py) with one worker against it — before
tests/test_random_des_gpu.py runs the engines on the same seeds."""
import functools

import numpy as np
import pytest

import isim
from isim import native
from oracle import des as od

import des_spans_ref as ref
import random_des_graphs as rd
import random_walk_graphs as rw
from test_random_walk import FEATURES


@functools.lru_cache(maxsize=None)
def oracle(family, seed, mode):
    """oracle.des.run over the case's N_SPANS window: (records, DES table)."""
    c = rd.case(family, seed, mode)
    orec, _, odes = od.run(c.sg, c.op, c.sg.entry(), c.begin, rd.N_SPANS, c.mean, og=c.og)
    return orec, odes


def test_recipe():
    """The draw as written down: replicas from one Random per graph over the walk family's graph, the mean by
    seed % 3, the walk family's parameters and window, pools from one Random per seed."""
    for family, seed in rd.CASES:
        doc, base = rd.des_graph(family, seed), rd.FAMILIES[family](seed)
        assert [s["numReplicas"] for s in doc["services"]] == [s["numReplicas"] for s in rd.des_graph(family, seed)["services"]]
        assert all(s["numReplicas"] in rd.REPLICAS for s in doc["services"])
        for s in doc["services"]:
            del s["numReplicas"]
        assert doc == base
    reps = [s["numReplicas"] for f, sd in rd.CASES for s in rd.des_graph(f, sd)["services"]]
    assert set(reps) == set(rd.REPLICAS)
    assert [rd.mean_ns(s) for s in (0, 1, 2, 3)] == [60_000, 300_000, 2_000_000, 60_000]
    assert rd.params(5, isim.MODE_B, native.FLAG_DYNAMIC) == \
        isim.SimParams(**{**rw.params(5, isim.MODE_B).__dict__, "flags": native.FLAG_DYNAMIC})
    assert rd.pool(7, 8) == rd.pool(7, 8) and len(rd.pool(7, 5)) == 5
    assert {w for s in rw.SEEDS for w in rd.pool(s, 8)} == {1, 2, 3, 4}
    assert rd.N_SPANS == 293 and rd.N_ORACLE == 1100 == 2 * 512 + 76


def test_class_census():
    """Creating a handler succeeds or raises EINVAL naming the unrolled tree, exactly where expected_refusal
    says (rd.census asserts both), and the classes are reached in the numbers the family was drawn for."""
    cen = rd.census()
    rd.check_census_counts(cen)
    assert rd.pooled_cases() == rd.POOLED and len(rd.POOLED) == 15
    # every refusal is a seed % 8 == 3 graph: a single sleep of 2^32 ns or more
    assert all(seed % 8 == 3 for (_, seed, _), v in cen.items() if v is None)
    assert sum(v is None for (f, _, m), v in cen.items() if f == "static" and m == isim.MODE_B) == 6
    assert sum(v is None for (f, _, _), v in cen.items() if f == "dynamic") == 12


def test_flag_variants():
    """Handlers only.  Every item-class case takes each flag the GPU tests serve it under; a level-class case
    forced dynamic moves to the item engine or is refused where expected_refusal says."""
    cen = rd.census()
    moved = refused = 0
    for (family, seed, mode), key in cen.items():
        if key is None:
            continue
        if key[0] == 1:
            for flags in (native.FLAG_TREE_WIDE, native.FLAG_DES_SCAN_BY_KEY, native.FLAG_DES_TWO_SORTS,
                          native.FLAG_DES_SORT_ALL, native.FLAG_DYNAMIC):
                assert rd.RandomDesCase(family, seed, mode, flags).d.info.items == 1
        elif rd.expected_refusal(family, seed, mode, native.FLAG_DYNAMIC):
            rd.assert_refused(family, seed, mode, native.FLAG_DYNAMIC)
            refused += 1
        else:
            assert rd.RandomDesCase(family, seed, mode, native.FLAG_DYNAMIC).d.info.items == 1
            moved += 1
    assert (moved, refused) == (66, 6)


def test_feature_census():
    """Every corner of the schema random_walk_graphs.features names is reached by at least 20 accepted cases."""
    seen = {f: 0 for f in FEATURES}
    for (family, seed, mode), key in rd.census().items():
        if key is not None:
            for f in rw.features(rd.des_graph(family, seed)):
                seen[f] += 1
    assert set(seen) == set(FEATURES)   # features() returned no name the list lacks
    assert min(seen.values()) >= 20, seen


@pytest.mark.parametrize("family,seed", rd.CASES, ids=rd.IDS)
def test_restatement_reproduces_the_oracle(family, seed):
    for mode in rd.MODES:
        if rd.census()[family, seed, mode] is None:
            continue
        c = rd.case(family, seed, mode)
        spans = rd.reference(family, seed, mode)
        orec, odes = oracle(family, seed, mode)
        assert np.array_equal(ref.latencies(spans), orec[:, 0]), mode
        assert np.array_equal(np.bincount(spans["trace"].astype(np.int64) - c.begin, minlength=rd.N_SPANS),
                              (orec[:, 1] & np.uint64(0xFFFFFFFF)).astype(np.int64)), mode
        entry = spans[spans["hop"] == 0]
        assert np.array_equal(entry["status"] & 1, (orec[:, 1] >> np.uint64(63)).astype(np.uint32)), mode
        t = ref.table_of(spans, len(c.sg.g.services))
        assert np.array_equal(t[:, 0], odes[:, native.DES_COUNT]), mode
        assert np.array_equal(t[:, 1], odes[:, native.DES_SUM_WAIT]), mode
        assert np.array_equal(t[:, 2], odes[:, native.DES_MAX_WAIT]), mode
        assert np.array_equal(t[:, 3], odes[:, 2 * native.N_PROM] + odes[:, 2 * native.N_PROM + 1]), mode


def test_contention_census():
    """At least 80 % of the accepted cases queue: a nonzero oracle DES_SUM_WAIT (measured: 160 of 174)."""
    accepted = [k for k, v in rd.census().items() if v is not None]
    waits = sum(int(oracle(*k)[1][:, native.DES_SUM_WAIT].sum()) > 0 for k in accepted)
    assert len(accepted) == 174 and waits >= 0.8 * len(accepted), waits


def test_pool_restatement():
    """On the acyclic item-engine cases: the pooled restatement with one worker everywhere is the spans
    restatement on every field, the handler takes the pool and reads it back, and the pool changes a start
    in at least 8 of the 15 (measured: 9)."""
    changed = 0
    for family, seed, mode in rd.POOLED:
        one = rd.reference(family, seed, mode)
        assert np.array_equal(rd.pooled_reference(family, seed, mode, ones=True), one), (family, seed, mode)
        c = rd.RandomDesCase(family, seed, mode)    # its own handler: the pool is the handler's state
        wl = rd.pool(seed, c.h.info.n_services)
        c.d.workers = wl
        assert c.d.workers.tolist() == wl
        pooled = rd.pooled_reference(family, seed, mode)
        assert len(pooled) == len(one)   # queueing changes no skip and no error: the same invocations
        changed += bool(np.any(pooled["start_ns"] != one["start_ns"]))
    assert changed >= 8, changed
