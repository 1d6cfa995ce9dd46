"""The reference of the DES worker-pool tests: the
event-driven restatement of tests/des_spans_ref.py with W_s workers per
replica.

One heap of ARRIVE events ordered (time, trace, hop), and per (service,
replica) a min-heap of W_s busy-until values: a request that arrives takes the
worker that frees first, start = max(time, heap[0]), and that worker is busy
until start + hold.  This is the pool as one would simulate it, NOT the stride
recurrence S_j = max(a_j, S_{j-W} + P) the device solves: the tests check the
recurrence against it (tests/test_des_workers.py).

With every W_s = 1 it is des_spans_ref.simulate row for row, which is pinned to
oracle/des_oracle.c (tests/test_des_spans.py).
"""
from __future__ import annotations

import heapq

import numpy as np

from oracle.executor_py import MODE_B
from oracle.philox import err_draw

from des_spans_ref import NONE, REF_DTYPE, _Tree, _word0, arrivals, holds, invocations, latencies, table_of  # noqa: F401


def simulate(sg, op, begin: int, n: int, arr: np.ndarray, workers, inv=None) -> np.ndarray:
    """Every executed invocation of the batch as a REF_DTYPE row, traces in order, hops in order; workers: per
    service index, the workers of each of its replicas."""
    inv = inv if inv is not None else invocations(sg, op, begin, n)
    modeb = op.error_mode == MODE_B
    nsvc = len(sg.g.services)
    workers = [int(w) for w in workers]
    assert len(workers) == nsvc and min(workers) >= 1
    reps = [max(1, s.num_replicas) for s in sg.g.services]
    hold = holds(sg)
    leaf = [not any(c[0] == "call" for step in sg.steps[s] for c in (step[1] if step[0] == "conc" else [step]))
            for s in range(nsvc)]
    tree = _Tree(sg)
    tree.subtree(sg.entry())
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(t) for t in inv])
    out = np.zeros(int(off[-1]), REF_DTYPE)
    pool = {}   # (service, replica) -> min-heap of its workers' busy-until times
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
        free = pool.get(key)
        if free is None:
            free = pool[key] = [0] * workers[svc]   # every worker idle at time 0 (a heap as it stands)
        start = max(time, free[0])
        heapq.heapreplace(free, start + hold[svc])  # the worker that frees first takes the request
        r["arrival_ns"], r["start_ns"] = time, start
        T[i][h] = start
        advance(i, h)
    return out
