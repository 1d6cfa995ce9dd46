"""GPU parity of the draw-stream walks' Philox round keys (stream_walk.h
philox_lockstep_from): round 3's keys are folded into its operands (the
batch's pre-xored c1 word; GroupEnt.d, from the group table or from the scalar
rounds in the kernel) and the keys of the later rounds are held in VGPRs per
batch or added up per group.  A wrong key or a wrong folded word changes every
draw of a block, so records, stats and per-site counters are compared
bit-exactly with the C oracle.

The cases run in two fresh child processes, one with the launch's group table
and one with ISIM_NO_GROUP_TABLE=1 (the library reads the switch when a handler
prepares the device), so that both producers of GroupEnt.d are compared with
the oracle; a child runs every case and reports one line per case, and the
tests below look their case up.  Within a child the oracle's result of a
(graph, mode, seed, range) is computed once and shared by the kernel variants.

Shapes: streams of 1, 3, 4, 5, 8 and 9 records (a last partial group and the
two padding groups), a group whose four records never err (the zero branch),
an errorRate-1 record, 261 records (66 groups: the 64-group chunk flush of
mode A), batches of 1, 127, 128, 129 and 389 traces (a wave walks 128), trace
ids from 0, from 2^32 - 64 (a batch straddling 2^32: a block per trace, and
the table refused past the crossing) and from 2^32 + 7, two seeds (one with
the high bit of both halves set: the key adds wrap).  Kernels: mode A (kind 4)
and mode B kinds 4, 5, 6 and 8 with the LDS counter table, and the global
counter variants of kinds 4 (both modes), 5 and 6 on graphs with more call
sites than the LDS table holds."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (1, 0x9E3779B9F4A7C15B)
TRACES = (1, 127, 128, 129, 389)
BEGINS = (0, (1 << 32) - 64, (1 << 32) + 7)
RANGES = [(b, n) for b in BEGINS for n in TRACES]
# the graphs of the global-counter kernels are large: one seed, the ragged
# two- and four-batch launches, with the table's t_hi and across 2^32
BIG_RANGES = [(0, 129), ((1 << 32) - 64, 389)]
BIG_LEAVES = 20600  # more call sites than the LDS counter table holds (8 B each in 160 KiB)

# name -> (error mode, flags, kernel kind)
VARIANTS = {
    "A": ("A", 0, 4),
    "B-mark": ("B", 0, 8),
    "B-closelist": ("B", "FLAG_CLOSE_LIST", 6),
    "B-bitstack": ("B", "FLAG_BIT_STACK", 5),
}


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


def _rates(records, zero_group=None, always=None):
    rates = [0.02 + 0.03 * (i % 5) for i in range(records - 1)]
    if zero_group is not None:  # records 4 g .. 4 g + 3 never err
        for r in range(4 * zero_group, 4 * zero_group + 4):
            rates[r - 1] = 0
    if always is not None:
        rates[always - 1] = 1.0
    return rates


def _graphs():
    g = {f"len{r}": (_star(_rates(r)), r) for r in (1, 3, 4, 5, 8, 9)}
    g["zero-group"] = (_star(_rates(12, zero_group=1)), 12)
    g["always"] = (_star(_rates(9, always=6)), 9)
    g["long"] = (_star(_rates(261, zero_group=2, always=18)), 261)
    return g


def _cases():
    """id -> (graph key, variant, kernel kind, lds_counters, seeds, ranges)"""
    c = {}
    for gk in _graphs():
        for v, (_, _, kind) in VARIANTS.items():
            c[f"{gk}-{v}"] = (gk, v, kind, 1, SEEDS, RANGES)
    # call depth 33: deeper than the bit stack, so its flag runs kind 4 in mode B
    c["deep-B-stack"] = ("deep", "B-bitstack", 4, 1, SEEDS, RANGES)
    c["big-A-global"] = ("big", "A", 4, 0, SEEDS[1:], BIG_RANGES)
    c["big-B-closelist-global"] = ("big", "B-closelist", 6, 0, SEEDS[1:], BIG_RANGES)
    c["big-B-bitstack-global"] = ("big", "B-bitstack", 5, 0, SEEDS[1:], BIG_RANGES)
    c["bigdeep-B-stack-global"] = ("bigdeep", "B-bitstack", 4, 0, SEEDS[1:], BIG_RANGES)
    return c


CASES = _cases()
SETTINGS = ("table", "no-table")


def _child():
    """Runs every case in this process; one line `id<TAB>ok|error` each."""
    import isim
    from parity import Case, assert_records_equal, assert_stats_equal
    from oracle import executor as oc

    graphs = {k: v[0] for k, v in _graphs().items()}
    graphs["deep"] = _chain(33, 2)
    graphs["big"] = _star([0.001 * (1 + i % 7) for i in range(BIG_LEAVES)])
    graphs["bigdeep"] = _chain(33, 650, leaf_rate=0.002)
    oracle = {}
    for cid, (gk, v, kind, lds, seeds, ranges) in CASES.items():
        try:
            mode, flags, _ = VARIANTS[v]
            for seed in seeds:
                c = Case(graphs[gk], None, isim.SimParams(
                    seed=seed, error_mode=isim.MODE_A if mode == "A" else isim.MODE_B,
                    flags=getattr(isim.native, flags) if flags else 0))
                info = c.handler.launch_info(0)
                assert c.handler.info.static_walk
                assert (info["kernel_kind"], info["lds_counters"]) == (kind, lds), (info["kernel_kind"],
                                                                                    info["lds_counters"])
                for begin, n in ranges:
                    key = (gk, mode, seed, begin, n)
                    if key not in oracle:
                        orec, ost = c.cpu(begin, n)
                        oracle[key] = (orec, oc.split_stats(ost, len(c.sg.g.services), len(c.sg.sites)))
                    recs, stats = c.gpu(begin, n)
                    try:
                        assert_records_equal(recs, oracle[key][0])
                        assert_stats_equal(c.handler.fold(stats), oracle[key][1])
                    except AssertionError as e:
                        raise AssertionError(f"seed {seed:#x} begin {begin:#x} n {n}: {e}") from None
            print(f"{cid}\tok", flush=True)
        except Exception as e:  # the case's line carries the failure to its test
            print(f"{cid}\t{type(e).__name__}: {str(e)[:300]}".replace("\n", " "), flush=True)


@pytest.fixture(scope="module")
def results(gpu):
    out = {}
    for setting in SETTINGS:
        env = dict(os.environ)
        env.pop("ISIM_NO_GROUP_TABLE", None)
        if setting == "no-table":
            env["ISIM_NO_GROUP_TABLE"] = "1"
        env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "istio-isotope_amd"), os.path.join(ROOT, "tests"),
                                             env.get("PYTHONPATH", "")])
        p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                           timeout=600)
        lines = dict(l.split("\t", 1) for l in p.stdout.splitlines() if "\t" in l)
        out[setting] = (p.returncode, lines, p.stderr[-2000:])
    return out


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("case", list(CASES))
def test_round_keys(results, case, setting):
    rc, lines, err = results[setting]
    assert case in lines, f"the child (exit {rc}) reported nothing for this case: {err}"
    assert lines[case] == "ok", lines[case]


if __name__ == "__main__":
    _child()
