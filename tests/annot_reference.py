"""CPU restatement of the annotation chain for the tests: ``scipy.stats.rankdata`` doubled
and cast to int64, Python integers for the sums, and the rho and quantile expressions exactly as the specification writes
them.  Besides the results it returns, per cell, the smallest decision margin met on the way: ``|score - (max - 0.05)|`` over
every label at every threshold test, and the gap between the top two scores at every argmax.  A case whose smallest margin
is far above the fp64 rounding of a score can be compared label for label, every cell included."""
import math

import numpy as np
from scipy.stats import rankdata

QUANTILE, TUNE_THRESH = 0.8, 0.05


def doubled_midranks(rows):
    """(r, m) values -> (r, m) int64: twice the midrank of every entry within its row (-0.0 == +0.0)"""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    if rows.shape[1] == 0:
        return np.zeros(rows.shape, dtype=np.int64)
    return np.rint(2.0 * rankdata(rows, method="average", axis=1)).astype(np.int64)


def integers(X, R):
    """-> sab (n, S), sa2 (n,), sb2 (S,) int64.  4 m^3 < 2^63 for every m the device accepts, so int64 holds them exactly."""
    A, B = doubled_midranks(X), doubled_midranks(R)
    return A @ B.T, (A * A).sum(axis=1), (B * B).sum(axis=1)


def rho(m, sab, sa2, sb2):
    m, sab, sa2, sb2 = int(m), int(sab), int(sa2), int(sb2)
    s = m * (m + 1)
    num, da, db = m * sab - s * s, m * sa2 - s * s, m * sb2 - s * s
    if da == 0 or db == 0:
        return 0.0
    return float(num) / math.sqrt(float(da) * float(db))


def quantile(c):
    c = sorted(float(v) for v in c)
    s = len(c)
    pos = QUANTILE * (s - 1)
    lo = math.floor(pos)
    return c[lo] + (pos - lo) * (c[min(lo + 1, s - 1)] - c[lo])


def label_scores(m, sab_row, sa2, sb2, ids, labels):
    """the scores of the labels `labels` for one cell; sab_row / sb2 indexed by sample"""
    out = {}
    for l in labels:
        out[l] = quantile([rho(m, sab_row[s], sa2, sb2[s]) for s in np.flatnonzero(ids == l)])
    return out


def scores(X, R, ids, L, row_of=None):
    """step 3: (n, L) fp64 scores and the argmax (lowest id on ties).  ``row_of``: see :func:`annotate`."""
    ids = np.asarray(ids)
    sab, sa2, sb2 = integers(X, R)
    if row_of is not None:
        sab, sb2 = sab[:, row_of], sb2[row_of]
    m = np.shape(X)[1]
    sc = np.empty((sab.shape[0], L), dtype=np.float64)
    for i in range(sab.shape[0]):
        row = label_scores(m, sab[i], sa2[i], sb2, ids, range(L))
        sc[i] = [row[l] for l in range(L)]
    return sc, np.argmax(sc, axis=1).astype(np.int32)


def _top_two(values):
    v = sorted(values, reverse=True)
    return v[0], (v[1] if len(v) > 1 else -math.inf)


def annotate(X, R, ids, L, pairs, trace=None, row_of=None):
    """Steps 3-5 on matrices restricted to the marker set M (n x m, S x m); ``pairs[(a, b)]``: positions in M.
    -> dict: scores, first_labels, labels, tuned_best, tuned_next, iterations, margin (n,), delta, pruned.
    ``trace`` (a list) receives ``(cell, use, |G'|)`` for every pass of the fine-tuning loop.  ``row_of``: R holds only the
    distinct sample rows and sample s is ``R[row_of[s]]`` (``ids`` has one entry per sample); a row's ranks depend on that
    row alone, so the integers of the distinct rows, indexed, are the integers of all the samples."""
    X, R, ids = np.asarray(X), np.asarray(R), np.asarray(ids)
    n = X.shape[0]
    sc, first = scores(X, R, ids, L, row_of)
    labels, iters = np.empty(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    best, nxt, margin = np.empty(n), np.empty(n), np.full(n, np.inf)
    ranked = {}                                    # use -> (G', the rows' doubled ranks over G', the samples' sums of squares)

    def reference_side(use):
        if use not in ranked:
            genes = sorted(set(int(j) for a in use for b in use if a != b for j in pairs[(a, b)]))
            B = doubled_midranks(R[:, genes])
            sb2 = (B * B).sum(axis=1)
            ranked[use] = (genes, B, sb2 if row_of is None else sb2[row_of])
        return ranked[use]

    def within(cur, i):
        mx = max(cur.values())
        thr = mx - TUNE_THRESH
        margin[i] = min(margin[i], min(abs(v - thr) for v in cur.values()))
        return tuple(l for l in sorted(cur) if cur[l] >= thr)

    for i in range(n):
        cur = {l: float(sc[i, l]) for l in range(L)}
        top, second = _top_two(cur.values())
        margin[i] = min(margin[i], top - second)                    # the argmax that gives first_labels
        use = within(cur, i)
        while len(use) > 1:
            genes, B, sb2 = reference_side(use)
            a = doubled_midranks(X[i, genes])[0]
            sab, sa2 = B @ a, int((a * a).sum())
            if row_of is not None:
                sab = sab[row_of]
            if trace is not None:
                trace.append((i, use, len(genes)))
            cur = label_scores(len(genes), sab, sa2, sb2, ids, use)
            iters[i] += 1
            new = within(cur, i)
            if new == use:
                break
            use = new
        top, second = _top_two(cur.values())
        margin[i] = min(margin[i], top - second)                    # the argmax that gives the label
        labels[i] = min(l for l in cur if cur[l] == top)
        best[i], nxt[i] = top, second
    delta, pruned = prune(sc, labels, best, nxt)
    return {"scores": sc, "first_labels": first, "labels": labels, "tuned_best": best, "tuned_next": nxt, "iterations": iters,
            "margin": margin, "delta": delta, "pruned": pruned}


def prune(sc, labels, best, nxt):
    delta = sc.max(axis=1) - np.median(sc, axis=1)
    pruned = np.zeros(len(labels), dtype=bool)
    for l in np.unique(labels):
        d = delta[labels == l]
        med = np.median(d)
        mad = np.median(np.abs(d - med))
        pruned[labels == l] = d < med - 3.0 * 1.4826 * mad
    return delta, pruned | ((best - nxt) < 0.0)


def brute_markers(R, ids, L, de_n):
    """step 2 by explicit loops: per ordered pair the genes by decreasing median difference, ties to the lower index"""
    R = np.asarray(R, dtype=np.float64)
    med = [np.median(R[np.asarray(ids) == l], axis=0) for l in range(L)]
    pairs = {}
    for a in range(L):
        for b in range(L):
            if a == b:
                continue
            order = sorted(range(R.shape[1]), key=lambda j: (-(med[a][j] - med[b][j]), j))[:de_n]
            pairs[(a, b)] = [j for j in order if med[a][j] - med[b][j] > 0]
    M = sorted(set(j for v in pairs.values() for j in v))
    return pairs, M
