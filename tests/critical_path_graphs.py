"""Graphs shared by tests/test_critical_path.py and tests/test_critical_path_gpu.py
(DESIGN.md §20): the ones of tests/test_spans_gpu.py that reach the 8-byte nodes,
the wide nodes, u64 time and the spilling chain, and a hand-written graph whose
concurrent steps reach every corner of the winner rule."""
import isim
from isim import native
from isim.generators import tree_topology
from isim.yamljson import obj_to_json


def _calls(doc):
    for s in doc["services"]:
        for st in s.get("script", []):
            for c in (st if isinstance(st, list) else [st]):
                if "call" in c:
                    yield c


def tree(sequential, prob=None, error_rate=0.1, sleep=None):
    doc = tree_topology(3, 3, sequential=sequential)
    for s in doc["services"]:
        s["errorRate"] = error_rate
        if sleep:
            s["script"] = [{"sleep": sleep}] + list(s.get("script") or [])
    for c in _calls(doc):
        if prob:
            c["call"] = {"service": c["call"] if isinstance(c["call"], str) else c["call"]["service"], "probability": prob}
    return doc


def chain(depth, prob=90):
    """c0 -> c1 -> ... each link also calling two leaves in one concurrent step, every call probabilistic."""
    svcs = []
    for i in range(depth):
        calls = [[{"call": {"service": n, "probability": prob}} for n in (f"c{i + 1}", f"l{i}-0", f"l{i}-1")]] \
            if i + 1 < depth else []
        svcs.append({"name": f"c{i}", "script": [{"sleep": "1us"}] + calls, "errorRate": 0.02})
        svcs += [{"name": f"l{i}-{j}", "errorRate": 0.03} for j in range(2)]
    svcs[0]["isEntrypoint"] = True
    return {"services": svcs}


def winners():
    """Every corner of the winner rule in one script.  Calls of one callee cost the same H + T, so:
    step 1 (two calls at 50 %): both skipped (no winner), the first skipped and the second wins, or a tie that
    the first wins; step 2: always a tie; step 3: its sleep outlasts m (and in mode B m's 500 fails the step);
    step 4: a sleep of 0 and a call at 30 %: no winner when the call is skipped (and, with free hops, a child
    of cost 0 that never wins when z runs and skips its own call); then a trailing call, so every step above
    is reached."""
    half = {"call": {"service": "l", "probability": 50}}
    return {"services": [
        {"name": "e", "isEntrypoint": True, "script": [
            [half, dict(half)], [{"call": "l"}, {"call": "l"}], [{"call": "m"}, {"sleep": "10ms"}],
            [{"sleep": "0s"}, {"call": {"service": "z", "probability": 30}}], {"call": "n"}]},
        {"name": "l", "script": [{"sleep": "1ms"}]},
        {"name": "m", "errorRate": 0.5, "script": [{"sleep": "2ms"}, {"call": "l"}]},
        {"name": "z", "script": [[{"call": {"service": "l", "probability": 20}}]]},
        {"name": "n", "script": [{"sleep": "3ms"}, [{"call": "l"}, {"call": "m"}]]},
    ]}


D, W = native.FLAG_DYNAMIC, native.FLAG_TREE_WIDE
# name -> (graph, flags); the comment names what the graph is there for
CASES = {
    "winners": (winners(), D),                               # the winner rule's corners
    "concurrent": (tree(False, prob=60), D),                 # 8-byte nodes, concurrent steps
    "chain40": (chain(40), D),                               # the spilling 40-deep chain (long, thin traces)
    "time64": (tree(True, prob=60, sleep="2s"), D),          # latency bound past 2^32 ns: u64 time
    "wide": (tree(False, prob=60), D | W),                   # 16-byte nodes
    "wide-winners": (winners(), D | W),
}


def make(name, mode, **kw):
    doc, flags = CASES[name]
    return isim.Handler(isim.ServiceGraph.from_json(obj_to_json(doc)), None,
                        isim.SimParams(error_mode=mode, flags=flags, **kw))


# ---- spans that are no walk's: the corruptions both test files refuse
CORRUPTIONS = ("hop", "caller_hop", "position", "service", "offsets")


def corrupt(kind, off, spans, victim, n_positions, n_services):
    """One trace of the list made something no walk writes; returns the list entries that must be refused."""
    a, b = int(off[victim]), int(off[victim + 1])
    assert b - a >= 3
    if kind == "hop":
        spans["hop"][a + 1] = 2
    elif kind == "caller_hop":
        spans["caller_hop"][a + 2] = 2
    elif kind == "position":
        spans["position"][b - 1] = n_positions
    elif kind == "service":
        spans["service"][a + 1] = n_services
    else:       # off[victim + 1] below off[victim]: the victim's range is empty, the next one's starts mid-trace
        off[victim + 1] = a - 1
        return [victim, victim + 1]
    return [victim]
