"""GPU parity on seeded random graphs over the schema's whole vocabulary
(tests/random_walk_graphs.py): every walk kernel path against the CPU oracle,
bit-exact records and folded stats (per-service durations included), in both
error modes, on 293 traces — for the draw stream two 128-trace batches and a
ragged one, for the other kernels four full waves and a ragged one.

The static family (probabilities absent, 0 or 100) reaches the draw-stream
kernels (kinds 4, 5, 6, 8), the interpreter (0/1) and, forced dynamic, the
lane tree walk (7) and the wave walk (2/3); its odd seeds are dynamic in mode
B by their aborts.  The dynamic family reaches kind 7 in its narrow and wide
formats and over the site graph, and the wave walk.  tests/test_random_walk.py
pins the generator and the oracle on the same seeds without a GPU."""
import dataclasses
import json

import pytest

import isim
import random_walk_graphs as rw
from isim.native import (FLAG_BIT_STACK, FLAG_CLOSE_LIST, FLAG_DYNAMIC, FLAG_NO_STREAM, FLAG_TREE_DAG,
                         FLAG_TREE_WIDE, FLAG_WAVE_WALK)
from parity import Case
from test_walk_gpu import dynamic_kind

pytestmark = pytest.mark.gpu

N_TRACES = 293
FAMILIES = {"static": rw.static_graph, "dynamic": rw.dynamic_graph}
PATHS = {"static": (0, FLAG_NO_STREAM, FLAG_BIT_STACK, FLAG_CLOSE_LIST, FLAG_DYNAMIC, FLAG_DYNAMIC | FLAG_WAVE_WALK),
         "dynamic": (0, FLAG_WAVE_WALK, FLAG_TREE_WIDE, FLAG_TREE_DAG)}
MODES = (isim.MODE_A, isim.MODE_B)
CASES = [(f, s, p) for f in FAMILIES for s in rw.SEEDS for p in PATHS[f]]


def make_case(family, seed, path, mode) -> Case:
    doc = FAMILIES[family](seed)
    return Case(json.dumps(doc), None, dataclasses.replace(rw.params(seed, mode), flags=path))


def expected_kind(handler, doc, path, mode):
    """(kernel_kind, tree_wide) of a handler: the rule of
    test_walk_gpu.test_reference_topologies for static walks, dynamic_kind for
    dynamic ones — where a single sleep reaches 2^32 ns there is no lane tree
    (include/isim.h, kernel_kind 7) and a dynamic walk takes the wave walk."""
    info = handler.info
    tb64 = int(info.time_bits == 64)
    if not info.static_walk:
        if rw.sleep_past_u32(doc):
            return 2 + tb64, 0
        kind = dynamic_kind(handler, path)
        wide = 2 if path & FLAG_TREE_DAG else 1 if path & FLAG_TREE_WIDE else 0
        return kind, wide if kind == 7 else 0
    if path & FLAG_NO_STREAM:
        return tb64, 0
    if mode == isim.MODE_A:
        return 4, 0
    if path & FLAG_BIT_STACK:
        return (5 if info.max_depth <= 32 else 4), 0
    return (6 if path & FLAG_CLOSE_LIST else 8), 0


@pytest.mark.parametrize("family,seed,path", CASES)
def test_random_graph(gpu, family, seed, path):
    doc = FAMILIES[family](seed)
    for mode in MODES:
        c = make_case(family, seed, path, mode)
        li = c.handler.launch_info(0)
        assert (li["kernel_kind"], li["tree_wide"]) == expected_kind(c.handler, doc, path, mode), (mode, li)
        c.compare(rw.window_begin(seed), N_TRACES)


def test_kind_census(gpu):
    """Handlers only, no launch: across the seeds every kernel kind, and kind 7
    in each of its three formats, is taken by at least 3 cases."""
    taken = {}
    for family, seed, path in CASES:
        doc = FAMILIES[family](seed)
        for mode in MODES:
            p = dataclasses.replace(rw.params(seed, mode), flags=path)
            h = isim.Handler(isim.ServiceGraph.from_json(json.dumps(doc)), None, p)
            li = h.launch_info(0)
            key = (li["kernel_kind"], li["tree_wide"])
            assert key == expected_kind(h, doc, path, mode), (family, seed, path, mode)
            taken.setdefault(key, set()).add((family, seed, path))
    want = [(k, 0) for k in (0, 1, 2, 3, 4, 5, 6, 8)] + [(7, 0), (7, 1), (7, 2)]
    counts = {key: len(taken.get(key, ())) for key in want}
    assert all(n >= 3 for n in counts.values()), counts
    assert set(taken) == set(want), sorted(taken)
