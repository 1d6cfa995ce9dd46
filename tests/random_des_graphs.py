"""Seeded random service graphs over the schema's whole vocabulary, for the
DES engines' parity tests (tests/test_random_des.py on the CPU,
tests/test_random_des_gpu.py on the GPU).

The graphs are those of tests/random_walk_graphs.py (probabilities 0, 1..99
and 100, negative sleeps, empty and sleep-only concurrent steps, empty scripts,
always-500 services in mid-tree, shared callees, sizes against response sizes,
hour-long sleeps) with a replica count drawn for every service; the walk
parameters and the window are that module's, the mean gap between arrivals
goes by the seed.  Everything is drawn from seeded random.Random objects alone,
so (family, seed) names a case for good.

isim.DesHandler decides a case's class on the host: the level engine (a static
walk), the item engine (a dynamic one), either with an acyclic or a cyclic
schedule, or no DES at all — a dynamic walk needs the lane tree walk's
unrolled tree, which a graph with a single sleep of 2^32 ns or more does not
have (expected_refusal).  census() reads the classes without a GPU.
"""
from __future__ import annotations

import dataclasses
import functools
import random

import isim
from isim.native import EINVAL, FLAG_DYNAMIC

import des_spans_ref as ref
import random_walk_graphs as rw
from test_des_gpu import DesCase

FAMILIES = {"static": rw.static_graph, "dynamic": rw.dynamic_graph}
MODES = (isim.MODE_A, isim.MODE_B)
CASES = [(f, s) for f in FAMILIES for s in rw.SEEDS]
IDS = [f"{f}-{s}" for f, s in CASES]
REPLICAS = (1, 1, 1, 2, 3, 5, 70)
MEANS = (60_000, 300_000, 2_000_000)
# the Python restatement's size: four waves and a ragged one, as the walk family's
N_SPANS = 293
# the C oracle's size: every trace executes the entry, so each round the entry
# feeds holds two 512-item k_qscan tiles and a ragged 76, and the level engine's
# replicated queue pass one 1,024-trace chunk and a tail
N_ORACLE = 1100


def des_graph(family: str, seed: int) -> dict:
    doc = FAMILIES[family](seed)
    rng = random.Random(f"des:{family}:{seed}")
    for svc in doc["services"]:
        svc["numReplicas"] = rng.choice(REPLICAS)
    return doc


def mean_ns(seed: int) -> int:
    return MEANS[seed % 3]


def params(seed: int, mode: int, flags: int = 0) -> isim.SimParams:
    return dataclasses.replace(rw.params(seed, mode), flags=flags)


def pool(seed: int, n_services: int) -> list:
    """Workers per replica of each service, by service index."""
    rng = random.Random(f"w:{seed}")
    return [rng.choice((1, 2, 3, 4)) for _ in range(n_services)]


def expected_refusal(family: str, seed: int, mode: int, flags: int = 0) -> bool:
    """No DES: a dynamic walk (by its probabilities, by mode-B aborts that skip
    steps, or forced) over a graph without an unrolled tree."""
    doc = des_graph(family, seed)
    dynamic = family == "dynamic" or bool(flags & FLAG_DYNAMIC) or \
        (mode == isim.MODE_B and rw.aborts_change_walk(doc["services"]))
    return dynamic and rw.sleep_past_u32(doc)


class RandomDesCase(DesCase):
    """DesCase of one (family, seed, error mode, flags): raises IsimError where expected_refusal says."""

    def __init__(self, family: str, seed: int, mode: int, flags: int = 0):
        self.family, self.seed, self.mode = family, seed, mode
        self.doc = des_graph(family, seed)
        self.begin = rw.window_begin(seed)
        super().__init__(self.doc, mean_ns(seed), **dataclasses.asdict(params(seed, mode, flags)))

    def key(self):
        """(item engine, cyclic schedule, the handler's time bits)."""
        return int(self.d.info.items), int(self.d.info.cyclic), int(self.h.info.time_bits)


def assert_refused(family: str, seed: int, mode: int, flags: int = 0) -> None:
    try:
        RandomDesCase(family, seed, mode, flags)
    except isim.IsimError as e:
        assert e.code == EINVAL and "unrolled tree" in str(e), (family, seed, mode, flags, str(e))
    else:
        raise AssertionError(f"{family}-{seed} mode {mode} flags {flags:#x}: a DES handler where none is expected")


@functools.lru_cache(maxsize=None)
def case(family: str, seed: int, mode: int, flags: int = 0) -> RandomDesCase:
    return RandomDesCase(family, seed, mode, flags)


@functools.lru_cache(maxsize=None)
def census() -> dict:
    """(family, seed, mode) -> RandomDesCase.key(), or None where the handler is refused; handlers only.
    A refusal is EINVAL naming the unrolled tree, and falls exactly where expected_refusal says."""
    out = {}
    for family, seed in CASES:
        for mode in MODES:
            if expected_refusal(family, seed, mode):
                assert_refused(family, seed, mode)
                out[family, seed, mode] = None
            else:
                out[family, seed, mode] = RandomDesCase(family, seed, mode).key()
    return out


def check_census_counts(cen: dict) -> None:
    """The class counts the family was drawn for (measured: 18 refusals; item engine 102, level engine 72;
    acyclic item engine 15; cyclic 87 and 46; 64-bit time 5 and 7)."""
    keys = [k for k in cen.values() if k is not None]
    assert len(cen) == 192 and len(cen) - len(keys) == 18
    items, level = [k for k in keys if k[0] == 1], [k for k in keys if k[0] == 0]
    assert len(items) >= 100 and len(level) >= 70, (len(items), len(level))
    assert sum(k[1] == 0 for k in items) >= 15
    assert sum(k[1] == 1 for k in items) >= 40 and sum(k[1] == 1 for k in level) >= 40
    assert sum(k[2] == 64 for k in items) >= 5 and sum(k[2] == 64 for k in level) >= 5


# the acyclic item-engine cases, the class isim_des_workers_set takes pools on, as (family, seed, mode):
# written out so that the tests over them are parametrised without building a handler; the census tests
# hold the list to pooled_cases()
POOLED = [("static", 7, isim.MODE_B)] + [("dynamic", s, m) for s in (1, 18, 20, 30, 36, 37, 41) for m in MODES]
POOLED_IDS = [f"{f}-{s}-{'ab'[m]}" for f, s, m in POOLED]


def pooled_cases() -> list:
    return [k for k, v in census().items() if v is not None and v[0] == 1 and v[1] == 0]


@functools.lru_cache(maxsize=None)
def invocations(family: str, seed: int, mode: int):
    c = case(family, seed, mode)
    return ref.invocations(c.sg, c.op, c.begin, N_SPANS)


@functools.lru_cache(maxsize=None)
def reference(family: str, seed: int, mode: int):
    """The one-worker restatement's spans of the case's N_SPANS window, computed once and never modified."""
    c = case(family, seed, mode)
    spans = ref.simulate(c.sg, c.op, c.begin, N_SPANS, ref.arrivals(c.op.seed, c.mean, c.begin, N_SPANS),
                         invocations(family, seed, mode))
    spans.setflags(write=False)
    return spans


@functools.lru_cache(maxsize=None)
def pooled_reference(family: str, seed: int, mode: int, ones: bool = False):
    """The pooled restatement's spans of the same window under pool(seed, ...), or with one worker everywhere."""
    import des_workers_ref as wref
    c = case(family, seed, mode)
    ns = len(c.sg.g.services)
    spans = wref.simulate(c.sg, c.op, c.begin, N_SPANS, ref.arrivals(c.op.seed, c.mean, c.begin, N_SPANS),
                          [1] * ns if ones else pool(seed, ns), invocations(family, seed, mode))
    spans.setflags(write=False)
    return spans
