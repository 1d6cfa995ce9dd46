"""A deliberately naive restatement of the service timeline: for every span and every row
the overlap max(0, min(y, hi) - max(x, lo)) on the integers.  No difference trick, no head and tail, no
division: independent of the host and of the device fold.  Two forms of the same formula: Python ints
(exact for every u64 input, slow) and int64 numpy blocks (times and row bounds below 2^62)."""
import numpy as np

ARRIVED, STARTED, FINISHED, SUM_WAIT, MAX_WAIT, QUEUED_NS, BUSY_NS, ROW_WORDS = 0, 1, 2, 4, 5, 6, 7, 8
H_FOLDED, H_REFUSED = 0, 1
M64 = (1 << 64) - 1


def row_bounds(window_ns, n_windows, t0_ns):
    """[lo, hi) per row as Python ints: before, the windows, after (which ends where u64 time ends)."""
    b = [(0, t0_ns)] + [(t0_ns + w * window_ns, t0_ns + (w + 1) * window_ns) for w in range(n_windows)]
    return b + [(t0_ns + n_windows * window_ns, 1 << 64)]


def refused(s, n_services):
    return int(s["service"]) >= n_services or not int(s["arrival_ns"]) <= int(s["start_ns"]) <= int(s["finish_ns"])


def fold_exact(spans, n_services, hold, window_ns, n_windows, t0_ns, table=None):
    """Python ints throughout; returns the flat table as Python ints mod 2^64 in a u64 array."""
    rows = row_bounds(window_ns, n_windows, t0_ns)
    R = len(rows)
    t = [0] * ((n_services * R + 1) * ROW_WORDS) if table is None else [int(x) for x in table]
    hdr = n_services * R * ROW_WORDS
    for s in spans:
        if refused(s, n_services):
            t[hdr + H_REFUSED] += 1
            continue
        t[hdr + H_FOLDED] += 1
        svc, a, S, F = int(s["service"]), int(s["arrival_ns"]), int(s["start_ns"]), int(s["finish_ns"])
        busy_end = min(S + int(hold[svc]), M64)
        for r, (lo, hi) in enumerate(rows):
            c = (svc * R + r) * ROW_WORDS
            t[c + ARRIVED] += lo <= a < hi
            if lo <= S < hi:
                t[c + STARTED] += 1
                t[c + SUM_WAIT] += S - a
                t[c + MAX_WAIT] = max(t[c + MAX_WAIT], S - a)
            if lo <= F < hi:
                t[c + FINISHED + (int(s["status"]) & 1)] += 1
            t[c + QUEUED_NS] += max(0, min(S, hi) - max(a, lo))
            t[c + BUSY_NS] += max(0, min(busy_end, hi) - max(S, lo))
    return np.array([x & M64 for x in t], dtype=np.uint64)


def fold(spans, n_services, hold, window_ns, n_windows, t0_ns, block=256):
    """The same formula on int64 numpy blocks of (spans x rows), into a zeroed table.  Every time, hold sum
    and row bound must lie below 2^62 (asserted); nothing is refused here (asserted)."""
    lim = 1 << 62
    bounds = row_bounds(window_ns, n_windows, t0_ns)
    bounds[-1] = (bounds[-1][0], lim)
    assert all(hi <= lim for _, hi in bounds)
    lo = np.array([b[0] for b in bounds], np.int64)[None, :]
    hi = np.array([b[1] for b in bounds], np.int64)[None, :]
    R = len(bounds)
    t = np.zeros((n_services, R, ROW_WORDS), np.int64)
    svc = spans["service"].astype(np.int64)
    a, S, F = (spans[f].astype(np.int64) for f in ("arrival_ns", "start_ns", "finish_ns"))
    assert len(spans) == 0 or (svc.max() < n_services and np.all(a <= S) and np.all(S <= F) and int(F.max()) < lim // 2)
    E = S + np.asarray(hold, np.int64)[svc]
    code = (spans["status"] & 1).astype(np.int64)
    for s in range(n_services):
        idx = np.flatnonzero(svc == s)
        for i in range(0, len(idx), block):
            j = idx[i:i + block]
            aa, SS, FF, EE, cc = a[j, None], S[j, None], F[j, None], E[j, None], code[j, None]
            t[s, :, ARRIVED] += ((lo <= aa) & (aa < hi)).sum(axis=0)
            st = (lo <= SS) & (SS < hi)
            t[s, :, STARTED] += st.sum(axis=0)
            t[s, :, SUM_WAIT] += (st * (SS - aa)).sum(axis=0)
            t[s, :, MAX_WAIT] = np.maximum(t[s, :, MAX_WAIT], (st * (SS - aa)).max(axis=0))
            fin = (lo <= FF) & (FF < hi)
            t[s, :, FINISHED] += (fin & (cc == 0)).sum(axis=0)
            t[s, :, FINISHED + 1] += (fin & (cc == 1)).sum(axis=0)
            t[s, :, QUEUED_NS] += np.maximum(0, np.minimum(SS, hi) - np.maximum(aa, lo)).sum(axis=0)
            t[s, :, BUSY_NS] += np.maximum(0, np.minimum(EE, hi) - np.maximum(SS, lo)).sum(axis=0)
    header = np.zeros(ROW_WORDS, np.int64)
    header[H_FOLDED] = len(spans)
    return np.concatenate([t.ravel(), header]).astype(np.uint64)
