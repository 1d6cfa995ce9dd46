"""The reference of the DES span tests: a plain event-driven
restatement of isim DES semantics v1 (§10.1) in Python that keeps what
oracle/des_oracle.c does not export, every invocation's arrival, start and
finish.

One heap of ARRIVE events ordered (time, trace, hop), one busy-until per
(service, replica).  The executed invocations of a trace come from the Python
oracle's event log (oracle/executor_py.py, as tests/test_spans.py takes them),
the arrival times from oracle.des's fixed-point exponential.  The restatement
is itself pinned (tests/test_des_spans.py): its latencies and its per-service
count, wait sum and wait maximum equal oracle.des.run's bit for bit on every
graph it is then used for.
"""
from __future__ import annotations

import heapq

import numpy as np

from oracle import des as od
from oracle.executor_py import MODE_B, run as py_run
from oracle.philox import err_draw, philox4x32_10

NONE = 0xFFFFFFFF
REF_DTYPE = np.dtype([("trace", "<u8"), ("arrival_ns", "<u8"), ("start_ns", "<u8"), ("finish_ns", "<u8"),
                      ("hop_ns", "<u8"), ("hop", "<u4"), ("caller_hop", "<u4"), ("position", "<u4"),
                      ("site", "<u4"), ("service", "<u4"), ("status", "<u4"), ("replica", "<u4")])


def _word0(seed, t, c2, c3):
    return philox4x32_10((t & 0xFFFFFFFF, t >> 32, c2, c3), (seed & 0xFFFFFFFF, seed >> 32))[0]


def arrivals(seed: int, mean_ns: int, begin: int, n: int) -> np.ndarray:
    """A_t of §10.1: the running sum of (mean * E(u_t)) >> 24, u_t word 0 of philox(t, 0, 0x80000001)."""
    out, now = np.zeros(n, np.uint64), 0
    for i in range(n):
        now += (mean_ns * od.exp_q24(_word0(seed, begin + i, 0, 0x80000001))) >> 24
        out[i] = now
    return out


def invocations(sg, op, begin: int, n: int):
    """Per trace the executed invocations in hop order as [service, status, caller hop, call site] (the entry:
    caller NONE, site NONE), from the event log: a recv opens an invocation under the innermost open one, a
    resp closes it, the sent that follows names the call site it was reached through."""
    _, st = py_run(sg, op, sg.entry(), begin, n, events=True)
    traces, cur, stack, closed = [], [], [], None
    for ev in st.events:
        if ev[0] == "recv":
            cur.append([ev[1], None, stack[-1] if stack else NONE, NONE])
            stack.append(len(cur) - 1)
        elif ev[0] == "resp":
            closed = stack.pop()
            assert cur[closed][0] == ev[1]
            cur[closed][1] = ev[3]
            if not stack:
                traces.append(cur)
                cur = []
        else:  # ("sent", caller, site): the call that just returned
            assert cur[cur[closed][2]][0] == ev[1]
            cur[closed][3] = ev[2]
    assert len(traces) == n and not cur
    return traces


class _Tree:
    """Sizes of the unrolled tree of potential invocations: a callee's position is its caller's + 1 + the
    subtrees of the caller's earlier call commands (preorder, call commands in script order)."""

    def __init__(self, sg):
        self.sg, self.size, self.before = sg, {}, {}

    def calls(self, s):
        for step in self.sg.steps[s]:
            for c in (step[1] if step[0] == "conc" else [step]):
                if c[0] == "call":
                    yield c[1]

    def subtree(self, s):
        if s not in self.size:
            n, b = 1, {}
            for site in self.calls(s):
                b[site] = n
                n += self.subtree(self.sg.sites[site][1])
            self.size[s], self.before[s] = n, b
        return self.size[s]


def holds(sg):
    """P_s of §10.1 per service: the sum of every sleep of its script, those of concurrent steps included."""
    return [sum(max(c[1], 0) for step in sg.steps[s] for c in (step[1] if step[0] == "conc" else [step])
                if c[0] == "sleep") for s in range(len(sg.g.services))]


def simulate(sg, op, begin: int, n: int, arr: np.ndarray, inv=None) -> np.ndarray:
    """Every executed invocation of the batch as a REF_DTYPE row, traces in order, hops in order."""
    inv = inv if inv is not None else invocations(sg, op, begin, n)
    modeb = op.error_mode == MODE_B
    nsvc = len(sg.g.services)
    reps = [max(1, s.num_replicas) for s in sg.g.services]
    hold = holds(sg)
    leaf = [not any(c[0] == "call" for step in sg.steps[s] for c in (step[1] if step[0] == "conc" else [step]))
            for s in range(nsvc)]
    tree = _Tree(sg)
    tree.subtree(sg.entry())
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(t) for t in inv])
    out = np.zeros(int(off[-1]), REF_DTYPE)
    busy = {}
    # per trace: kids[hop][site] = the callee's hop; the script state of each invocation
    kids = [[{} for _ in t] for t in inv]
    for i, t in enumerate(inv):
        for h, (svc, status, caller, site) in enumerate(t):
            r = out[off[i] + h]
            r["trace"], r["hop"], r["caller_hop"], r["site"], r["service"] = begin + i, h, caller, site, svc
            own = status and (not modeb or leaf[svc] or sg.thr[svc] >= (1 << 32) or
                              (sg.thr[svc] > 0 and err_draw(op.seed, begin + i, h) < sg.thr[svc]))
            r["status"] = (1 if status else 0) | (2 if own else 0)
            if h:
                kids[i][caller][site] = h
                r["hop_ns"] = sg.hop_cost(site, op)
                r["position"] = out[off[i] + caller]["position"] + tree.before[t[caller][0]][site]
            r["replica"] = _word0(op.seed, begin + i, h, 0x80000002) % reps[svc] if reps[svc] > 1 else 0
    T = [[0] * len(t) for t in inv]
    runmax = [[0] * len(t) for t in inv]
    step = [[0] * len(t) for t in inv]
    pending = [[0] * len(t) for t in inv]
    failing = [[False] * len(t) for t in inv]
    heap = [(int(arr[i]), begin + i, 0) for i in range(n)]
    heapq.heapify(heap)

    def send(i, h, site):
        c = kids[i][h].get(site)
        if c is None:
            return
        heapq.heappush(heap, (T[i][h] + sg.hop_cost(site, op), begin + i, c))
        pending[i][h] += 1
        if modeb and inv[i][c][1]:
            failing[i][h] = True

    def advance(i, h):
        while True:
            steps = sg.steps[inv[i][h][0]]
            done = True
            while step[i][h] < len(steps) and not failing[i][h]:
                st = steps[step[i][h]]
                step[i][h] += 1
                if st[0] == "sleep":
                    T[i][h] += max(st[1], 0)
                    continue
                if st[0] == "call":
                    runmax[i][h] = T[i][h]
                    send(i, h, st[1])
                else:
                    runmax[i][h] = T[i][h] + max([max(c[1], 0) for c in st[1] if c[0] == "sleep"] or [0])
                    for c in st[1]:
                        if c[0] == "call":
                            send(i, h, c[1])
                if pending[i][h]:
                    done = False
                    break
                T[i][h] = runmax[i][h]
            if not done:
                return
            out[off[i] + h]["finish_ns"] = T[i][h]
            p = inv[i][h][2]
            if p == NONE:
                return
            # the response reaches the caller at this finish; its step ends with its last callee
            runmax[i][p] = max(runmax[i][p], T[i][h])
            pending[i][p] -= 1
            if pending[i][p]:
                return
            T[i][p] = runmax[i][p]
            h = p

    while heap:
        time, trace, h = heapq.heappop(heap)
        i = trace - begin
        svc = inv[i][h][0]
        r = out[off[i] + h]
        key = (svc, int(r["replica"]))
        start = max(time, busy.get(key, 0))
        busy[key] = start + hold[svc]
        r["arrival_ns"], r["start_ns"] = time, start
        T[i][h] = start
        advance(i, h)
    return out


def table_of(spans: np.ndarray, n_services: int) -> np.ndarray:
    """[n_services][4]: count, sum of waits, max wait, sum of F - a per service."""
    t = np.zeros((n_services, 4), np.uint64)
    w = spans["start_ns"] - spans["arrival_ns"]
    for s in range(n_services):
        m = spans["service"] == s
        if m.any():
            t[s] = (m.sum(), w[m].sum(), w[m].max(), (spans["finish_ns"] - spans["arrival_ns"])[m].sum())
    return t


def latencies(spans: np.ndarray) -> np.ndarray:
    e = spans[spans["hop"] == 0]
    return e["finish_ns"] - e["arrival_ns"]
