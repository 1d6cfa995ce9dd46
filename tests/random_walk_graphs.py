"""Seeded random service graphs over the schema's whole vocabulary, for the
walk's parity tests (tests/test_random_walk.py on the CPU,
tests/test_random_walk_gpu.py on the GPU).

Everything is drawn from random.Random(seed) alone, so a seed names a graph
for good.  Two families:

  static_graph(seed)   every call has probability absent, 0 or 100 (all
                       "always": program.cpp takes only 1..99 as "maybe"), so
                       the walk is static in mode A — the draw-stream kernels
                       (kinds 4, 5, 6, 8) and the interpreter (0/1).  Even
                       seeds are shaped so that no step follows a step that
                       can fail (static in mode B too); odd seeds have such a
                       step (dynamic in mode B).
  dynamic_graph(seed)  probabilities from {0, 1, 30, 50, 99, 100} with at
                       least one of 1..99 on a path from the entry — the lane
                       tree walk (kind 7) and the wave walk (2/3).

Services are s0..s(n-1), s0 the entry, calls go to higher indices only.  The
generator bounds the unrolled tree itself: while the potential invocations
from the entry pass MAX_INVOCATIONS it draws again from the same Random.
Seeds with seed % 8 == 3 give one reachable service a sleep of hours (a
latency bound past 2^32 ns: 64-bit time).

features(doc) names the corners of the schema a graph reaches (over the
services reachable from the entry); the tests take a census of them.
"""
from __future__ import annotations

import random

import isim

MAX_INVOCATIONS = 2048
ERROR_RATES = (0, 0.001, 0.1, 0.5, 1.0)
STATIC_PROBS = (None, 0, 100)
DYNAMIC_PROBS = (None, 0, 1, 30, 50, 99, 100)
SEEDS = range(48)
# weights: from one service and a handful of invocations to trees of hundreds
N_SERVICES = (1, 2, 3, 4, 5, 6, 6, 7, 7, 8, 8, 8)
N_STEPS = (0, 1, 2, 3, 3, 4, 4, 4)
STEP_KINDS = ("sleep", "call", "call", "conc", "conc")


# ---- reading a generated graph -------------------------------------------

def _index(name: str) -> int:
    return int(name[1:])


def _call_of(cmd: dict):
    """(callee index, size or None, probability or None) of a call command."""
    c = cmd["call"]
    if isinstance(c, str):
        return _index(c), None, None
    return _index(c["service"]), c.get("size"), c.get("probability")


def step_calls(step) -> list:
    """The call commands of one step (a sleep: none; a concurrent step: its members')."""
    members = step if isinstance(step, list) else [step]
    return [m for m in members if "call" in m]


def _callees(svc: dict) -> list:
    return [_call_of(c)[0] for step in svc["script"] for c in step_calls(step)]


def reachable(services: list) -> list:
    seen, todo = {0}, [0]
    while todo:
        for c in _callees(services[todo.pop()]):
            if c not in seen:
                seen.add(c)
                todo.append(c)
    return sorted(seen)


def invocations(services: list) -> int:
    """Potential invocations per trace from the entry (every call made)."""
    count = [0] * len(services)
    for i in reversed(range(len(services))):  # callees have higher indices
        count[i] = 1 + sum(count[c] for c in _callees(services[i]))
    return count[0]


def fallible(services: list) -> list:
    """Per service: can an invocation respond 500 in mode B (its own errorRate
    or, through an abort, a callee's)."""
    f = [False] * len(services)
    for i in reversed(range(len(services))):
        f[i] = services[i]["errorRate"] > 0 or any(f[c] for c in _callees(services[i]))
    return f


def aborts_change_walk(services: list) -> bool:
    """Mode B: some reachable script has a step after a step that can fail, so
    a failure skips invocations (the walk is not static)."""
    f = fallible(services)
    for i in reachable(services):
        script = services[i]["script"]
        for step in script[:-1]:
            if any(f[_call_of(c)[0]] for c in step_calls(step)):
                return True
    return False


def _maybe(services: list) -> bool:
    return any(p is not None and 1 <= p <= 99 for i in reachable(services)
               for step in services[i]["script"] for c in step_calls(step) for p in [_call_of(c)[2]])


def _sleep_ns(text: str) -> int:
    for unit, ns in (("ms", 10 ** 6), ("h", 3600 * 10 ** 9)):
        if text.endswith(unit):
            return int(text[:-len(unit)]) * ns
    raise ValueError(text)


def sleep_past_u32(doc: dict) -> bool:
    """A reachable service sleeps 2^32 ns or longer in one command: such a walk
    has no lane tree (include/isim.h, kernel_kind), dynamic walks take kinds 2/3."""
    services = doc["services"]
    for i in reachable(services):
        for step in services[i]["script"]:
            for m in (step if isinstance(step, list) else [step]):
                if "sleep" in m and _sleep_ns(m["sleep"]) >= 1 << 32:
                    return True
    return False


def features(doc: dict) -> set:
    """The schema corners a graph reaches, over the services reachable from the entry."""
    services = doc["services"]
    out = set()
    for i in reachable(services):
        svc = services[i]
        if not svc["script"]:
            out.add("empty_script")
        if i != 0 and svc["errorRate"] == 1.0 and _callees(svc):
            out.add("always_500_mid_tree")
        callees = _callees(svc)
        if len(set(callees)) < len(callees):
            out.add("callee_from_several_sites")
        for step in svc["script"]:
            if isinstance(step, list):
                if not step:
                    out.add("empty_concurrent")
                elif not step_calls(step):
                    out.add("concurrent_only_sleeps")
                if any("sleep" in m and _sleep_ns(m["sleep"]) < 0 for m in step):
                    out.add("negative_sleep_in_concurrent")
            for c in step_calls(step):
                callee, size, prob = _call_of(c)
                if prob == 0:
                    out.add("probability_0")
                if prob == 100:
                    out.add("probability_100")
                if size is not None and services[callee]["responseSize"] > 0:
                    out.add("size_with_response_size")
    return out


# ---- drawing ----------------------------------------------------------------

def _draw_call(rng: random.Random, i: int, n: int, probs) -> dict:
    # the next service half the time: deep chains, most services on a path from the entry
    c = {"service": f"s{i + 1 if rng.random() < 0.5 else rng.randint(i + 1, n - 1)}"}
    if rng.random() < 0.5:
        c["size"] = rng.randint(0, 5000)
    p = rng.choice(probs)
    if p is not None:
        c["probability"] = p
    return {"call": c if len(c) > 1 else c["service"]}


def _draw_services(rng: random.Random, probs) -> list:
    n = rng.choice(N_SERVICES)
    services = []
    for i in range(n):
        steps = []
        for _ in range(rng.choice(N_STEPS)):
            kind = rng.choice(STEP_KINDS)
            if kind == "sleep":
                steps.append({"sleep": f"{rng.randint(-2, 40)}ms"})
            elif kind == "call":
                if i + 1 < n:
                    steps.append(_draw_call(rng, i, n, probs))
            else:
                members = []
                for _ in range(rng.randint(0, 3)):
                    if i + 1 < n and rng.random() < 0.65:
                        members.append(_draw_call(rng, i, n, probs))
                    else:
                        members.append({"sleep": f"{rng.randint(-2, 9)}ms"})
                steps.append(members)
        services.append({"name": f"s{i}", "script": steps, "errorRate": rng.choice(ERROR_RATES),
                         "responseSize": rng.randint(0, 100000)})
    services[0]["isEntrypoint"] = True
    return services


def _retarget(cmd: dict, callee: int) -> None:
    if isinstance(cmd["call"], str):
        cmd["call"] = f"s{callee}"
    else:
        cmd["call"]["service"] = f"s{callee}"


def _clear_errors(services: list, s: int) -> None:
    services[s]["errorRate"] = 0
    for c in _callees(services[s]):
        _clear_errors(services, c)


def _shape_static_in_mode_b(rng: random.Random, services: list) -> None:
    """No step follows a step that can fail: one such step of a script moves to
    its end; the calls of the others go to callees below which every errorRate
    is 0, or every errorRate below them becomes 0."""
    n = len(services)
    for i in reversed(range(n)):
        script = services[i]["script"]
        f = fallible(services)  # of the services above i: already shaped
        bad = [step for step in script if any(f[_call_of(c)[0]] for c in step_calls(step))]
        if not bad:
            continue
        last = rng.choice(bad)
        script[:] = [step for step in script if step is not last] + [last]
        for step in script[:-1]:
            for c in step_calls(step):
                f = fallible(services)
                safe = [x for x in range(i + 1, n) if not f[x]]
                if not f[_call_of(c)[0]]:
                    continue
                if safe and rng.random() < 0.5:
                    _retarget(c, rng.choice(safe))
                else:
                    _clear_errors(services, _call_of(c)[0])


def _graph(seed: int, family: str) -> dict:
    rng = random.Random(f"{family}:{seed}")
    dynamic = family == "dynamic"
    shaped = not dynamic and seed % 2 == 0
    while True:
        services = _draw_services(rng, DYNAMIC_PROBS if dynamic else STATIC_PROBS)
        if shaped:
            _shape_static_in_mode_b(rng, services)
        if invocations(services) > MAX_INVOCATIONS:
            continue
        if dynamic and not _maybe(services):
            continue
        if not dynamic and shaped == aborts_change_walk(services):
            continue  # an unshaped seed has a step after one that can fail
        break
    if seed % 8 == 3:  # first in its script: it follows no step
        services[rng.choice(reachable(services))]["script"].insert(0, {"sleep": f"{rng.randint(1, 3)}h"})
    return {"defaults": {"requestSize": 100}, "services": services}


def static_graph(seed: int) -> dict:
    return _graph(seed, "static")


def dynamic_graph(seed: int) -> dict:
    return _graph(seed, "dynamic")


def params(seed: int, mode: int) -> isim.SimParams:
    rng = random.Random(f"params:{seed}")
    return isim.SimParams(seed=rng.getrandbits(64), hop_base_ns=rng.choice((0, 250_000, 1)),
                          req_ps_per_byte=rng.choice((0, 80, 10 ** 6)), resp_ps_per_byte=rng.choice((0, 80, 10 ** 6)),
                          error_mode=mode)


def window_begin(seed: int) -> int:
    """First trace id of a seed's window: for seeds divisible by 8 the ids straddle 2^32."""
    return (1 << 32) - 150 if seed % 8 == 0 else seed * 1_000_003
