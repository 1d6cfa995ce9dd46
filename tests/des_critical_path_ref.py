"""The reference of the DES critical path tests: a recursive
Python restatement of the rule over des_spans_ref.simulate's rows and the
graph's scripts.  It keeps its own clock per caller, takes the call index of a
child from its call site's place among the caller's call commands, and shares
no code with the C++ fold.
"""
from __future__ import annotations

import sys

import numpy as np

NONE = 0xFFFFFFFF
ROW_WORDS = 8
INVOCATIONS, SUM_DURATION, CRITICAL, WAIT_NS, SELF_NS, HOP_NS, CRITICAL_500, CRITICAL_WAITED = range(8)
H_TRACES, H_SPANS, H_CRITICAL, H_SUM_LATENCY, H_REFUSED = range(5)
U64_MAX = (1 << 64) - 1


class Refused(Exception):
    pass


def call_index(sg):
    """Per service {site: its index among the service's call commands in script order}."""
    out = []
    for steps in sg.steps:
        k, d = 0, {}
        for step in steps:
            for c in (step[1] if step[0] == "conc" else [step]):
                if c[0] == "call":
                    d[c[1]] = k
                    k += 1
        out.append(d)
    return out


def fold_trace(sg, rows, n_positions, kidx=None, equations=None, corners=None):
    """One trace's rows (any structured array with des_spans_ref.REF_DTYPE's fields, in hop order).  Returns
    (critical[m] bool, self[m] int) or raises Refused.  equations: a list that takes (child row index, clock +
    hop_ns) of every matched child, whether the arrival equation holds or not.  corners: a Counter of what the
    concurrent steps of critical callers met (a sleep won, a tie, a first call skipped and a later one winning,
    no winner)."""
    kidx = kidx or call_index(sg)
    m = len(rows)
    nsvc = len(sg.g.services)
    a = [int(x) for x in rows["arrival_ns"]]
    S = [int(x) for x in rows["start_ns"]]
    F = [int(x) for x in rows["finish_ns"]]
    H = [int(x) for x in rows["hop_ns"]]
    caller = [int(x) for x in rows["caller_hop"]]
    site = [int(x) for x in rows["site"]]
    svc = [int(x) for x in rows["service"]]
    for j in range(m):
        if int(rows["hop"][j]) != j or int(rows["position"][j]) >= n_positions or svc[j] >= nsvc:
            raise Refused("hop, position or service")
        if not a[j] <= S[j] <= F[j]:
            raise Refused("times")
        if j == 0:
            if caller[0] != NONE or H[0] != 0:
                raise Refused("entry")
            continue
        if caller[j] >= j:
            raise Refused("forward caller")
        anc = j - 1     # preorder: the caller of j is j - 1 or one of its callers
        while anc > caller[j]:
            anc = caller[anc]
        if anc != caller[j]:
            raise Refused("not in preorder")
    kids = [[] for _ in range(m)]
    for j in range(1, m):
        kids[caller[j]].append(j)
    critical = np.zeros(m, bool)
    self_ns = [0] * m

    def visit(v, crit):
        critical[v] = crit
        clock = S[v]
        todo = list(kids[v])
        k = 0
        winners, won = set(), 0

        def take():
            nonlocal k
            kk = k
            k += 1
            if not todo or kidx[svc[v]].get(site[todo[0]]) != kk:
                return None
            c = todo.pop(0)
            if equations is not None:
                equations.append((c, clock + H[c]))
            if a[c] != clock + H[c]:
                raise Refused("arrival equation")
            return c

        for step in sg.steps[svc[v]]:
            if not todo:
                break    # (mode B: nothing follows a failed step; otherwise only sleeps are left)
            if step[0] == "sleep":
                clock += max(step[1], 0)
            elif step[0] == "call":
                c = take()
                if c is not None:
                    winners.add(c)
                    won += H[c] + F[c] - a[c]
                    clock += H[c] + F[c] - a[c]
            else:
                longest, winner, tie, first_skipped, seen_call = 0, None, False, False, False
                for mem in step[1]:
                    if mem[0] == "call":
                        c = take()
                        val, who = (H[c] + F[c] - a[c], c) if c is not None else (0, None)
                    else:
                        val, who = (max(mem[1], 0) if mem[0] == "sleep" else 0), "sleep"
                    if mem[0] == "call":
                        first_skipped |= not seen_call and who is None
                        seen_call = True
                    tie |= val == longest and val > 0
                    if val > longest:
                        longest, winner, tie = val, who, False
                if corners is not None and crit:
                    corners["sleep_won"] += winner == "sleep"
                    corners["tie"] += tie
                    corners["no_winner"] += winner is None
                    corners["skipped_then_later"] += first_skipped and winner not in (None, "sleep")
                if winner is not None and winner != "sleep":
                    winners.add(winner)
                    won += longest
                clock += longest
        if todo:
            raise Refused("a child without a call command")
        self_ns[v] = F[v] - S[v] - won
        if self_ns[v] < 0:
            raise Refused("negative self")
        for c in kids[v]:
            visit(c, crit and c in winners)

    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 4 * m + 100))
    try:
        visit(0, True)
    finally:
        sys.setrecursionlimit(old)
    return critical, self_ns


def fold(sg, rows, off, n_positions, equations=None, corners=None):
    """A list of traces: (status bits to OR per row, table[(S + 1), 8] as Python ints mod 2^64, per-trace
    critical wait with U64_MAX for a refused trace)."""
    nsvc = len(sg.g.services)
    kidx = call_index(sg)
    table = [[0] * ROW_WORDS for _ in range(nsvc + 1)]
    bits = np.zeros(len(rows), np.uint32)
    waits = []
    for i in range(len(off) - 1):
        lo, hi = int(off[i]), int(off[i + 1])
        try:
            if hi <= lo or hi > int(off[-1]):
                raise Refused("offsets")
            eq = [] if equations is not None else None
            crit, self_ns = fold_trace(sg, rows[lo:hi], n_positions, kidx, eq, corners)
            if equations is not None:
                equations += [(lo + c, want) for c, want in eq]
        except Refused:
            table[nsvc][H_REFUSED] += 1
            waits.append(U64_MAX)
            continue
        r = rows[lo:hi]
        hdr = table[nsvc]
        hdr[H_TRACES] += 1
        hdr[H_SPANS] += hi - lo
        hdr[H_SUM_LATENCY] += int(r["finish_ns"][0]) - int(r["arrival_ns"][0])
        w = 0
        for j in range(hi - lo):
            row = table[int(r["service"][j])]
            a, S, F = int(r["arrival_ns"][j]), int(r["start_ns"][j]), int(r["finish_ns"][j])
            row[INVOCATIONS] += 1
            row[SUM_DURATION] += F - a
            if crit[j]:
                bits[lo + j] = 4
                hdr[H_CRITICAL] += 1
                row[CRITICAL] += 1
                row[WAIT_NS] += S - a
                row[SELF_NS] += self_ns[j]
                row[HOP_NS] += int(r["hop_ns"][j])
                row[CRITICAL_500] += int(r["status"][j]) & 1
                row[CRITICAL_WAITED] += 1 if S > a else 0
                w += S - a
        waits.append(w)
    t = np.array([[x % (1 << 64) for x in row] for row in table], np.uint64)
    return bits, t, np.array(waits, np.uint64)
