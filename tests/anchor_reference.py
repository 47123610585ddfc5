"""numpy restatement of chain A (kernels: csrc/anchor_kernels.hip): anchor-based label and feature
transfer, Seurat v4's FindAnchorPairs / ScoreAnchors / FindWeights / TransferData as this package specifies them.  TEST
INFRASTRUCTURE ONLY: nothing in the package imports it.  Written from the specification, stage by stage, so that a test can
feed a stage the device's previous output.

A1 ranks by chain Q1's f32 distance chain (mapping_reference.chain_d2), ascending (d2, index); A2 and A3 are integer set
operations; A5 and A6 are fp64, every sum taken in the stated order (np.cumsum / np.add.at / explicit loops: never np.sum,
whose pairwise order is numpy's own)."""
import numpy as np

import mapping_reference as mref


# ---- A0 -----------------------------------------------------------------------------------------------------------------------

def l2_normalize(X):
    """every row divided by its fp64 Euclidean norm (sum of squares in coordinate order), rounded to f32"""
    X = np.asarray(X, dtype=np.float32)
    x = X.astype(np.float64)
    ss = np.zeros(len(x))
    for c in range(x.shape[1]):
        ss = ss + x[:, c] * x[:, c]
    if not (ss > 0).all():
        raise ValueError("an all-zero row")
    return (x / np.sqrt(ss)[:, None]).astype(np.float32)


# ---- A1 -----------------------------------------------------------------------------------------------------------------------

def cross_knn(Q, R, k, chunk=512):
    """mapping_reference.cross_knn in chunks of queries: (m, k) indices into R by ascending (chain d2, index).  A
    non-negative f32 orders as its bit pattern, so (bits << 32 | index) is one integer key per pair."""
    Q, R = np.asarray(Q, dtype=np.float32), np.asarray(R, dtype=np.float32)
    n = len(R)
    out = np.empty((len(Q), k), dtype=np.int32)
    cols = np.arange(n, dtype=np.int64)
    for a in range(0, len(Q), chunk):
        q = Q[a:a + chunk]
        d2 = mref.chain_d2(q, R, np.broadcast_to(np.arange(n), (len(q), n)))
        key = (d2.view(np.int32).astype(np.int64) << 32) | cols
        if k < n:
            key = np.partition(key, k - 1, axis=1)[:, :k]
        out[a:a + chunk] = (np.sort(key, axis=1) & 0xFFFFFFFF).astype(np.int32)
    return out


def knn_tables(R, Q, K):
    """(RR, RQ, QR, QQ): reference in reference, reference in query (n x K), query in reference, query in query (m x K);
    nothing excluded"""
    return cross_knn(R, R, K), cross_knn(R, Q, K), cross_knn(Q, R, K), cross_knn(Q, Q, K)


# ---- A2 -----------------------------------------------------------------------------------------------------------------------

def anchor_pairs(RQ, QR, k_anchor):
    """(A, 2) int32 (r, q): q in RQ[r, :k_anchor] and r in QR[q, :k_anchor]; by ascending r, then q's rank in RQ[r]"""
    fwd = np.asarray(RQ)[:, :k_anchor]                            # (n, ka): q
    back = np.asarray(QR)[:, :k_anchor][fwd]                      # (n, ka, ka): the reference cells q lists
    mutual = (back == np.arange(len(fwd))[:, None, None]).any(axis=2)
    r, p = np.nonzero(mutual)                                     # row-major: ascending r, then rank
    return np.stack([r, fwd[r, p]], axis=1).astype(np.int32)


# ---- A3 -----------------------------------------------------------------------------------------------------------------------

def anchor_raw(pairs, RR, RQ, QR, QQ, k_score, chunk=2048):
    """raw = |S_r n S_q|, S_r = RR[r, :ks] u (n + RQ[r, :ks]), S_q = QR[q, :ks] u (n + QQ[q, :ks])"""
    n = len(RR)
    raw = np.empty(len(pairs), dtype=np.int32)
    for a in range(0, len(pairs), chunk):
        r, q = pairs[a:a + chunk, 0], pairs[a:a + chunk, 1]
        s_r = np.concatenate([RR[r, :k_score], n + RQ[r, :k_score]], axis=1)
        s_q = np.concatenate([QR[q, :k_score], n + QQ[q, :k_score]], axis=1)
        raw[a:a + chunk] = (s_r[:, :, None] == s_q[:, None, :]).any(axis=2).sum(axis=1)
    return raw


def normalize_scores(raw):
    """clip((raw - lo) / (hi - lo), 0, 1), lo, hi = the 0.01 and 0.90 quantiles; hi == lo: every score is 1"""
    raw = np.asarray(raw, dtype=np.float64)
    lo, hi = np.quantile(raw, [0.01, 0.90])
    if hi == lo:
        return np.ones(len(raw))
    return np.clip((raw - lo) / (hi - lo), 0.0, 1.0)


# ---- A4 -----------------------------------------------------------------------------------------------------------------------

def anchor_queries(pairs):
    """U: the distinct query cells of the anchors, ascending"""
    return np.unique(np.asarray(pairs)[:, 1]).astype(np.int32)


def weight_knn(Q, U, k_weight):
    """(WN, WD): for every query cell its k_weight nearest rows of Q[U] (indices into U) and Q1's f32 distances"""
    if k_weight > len(U):
        raise ValueError("k_weight = %d exceeds |U| = %d" % (k_weight, len(U)))
    Q = np.asarray(Q, dtype=np.float32)
    WN = cross_knn(Q, Q[U], k_weight)
    return WN, mref.distances(Q, Q[U], WN, "euclidean")


# ---- A5 -----------------------------------------------------------------------------------------------------------------------

def compensated_sum(w):
    """the sum of w left to right with Neumaier's compensation, fp64: s and the running error term, added at the end"""
    s = comp = 0.0
    for x in (float(v) for v in w):
        t = s + x
        comp += (s - t) + x if abs(s) >= abs(x) else (x - t) + s
        s = t
    return s + comp


def anchor_weights(pairs, score, m, U, WN, WD, sd_weight=1.0):
    """CSR (rowptr int64, anchor int32, weight fp64): row c walks i = 0 .. k_weight - 1 and, for each, the anchors of query cell
    U[WN[c, i]] in anchor-list order; t = (1 - WD[c, i] / dk) * score[a] (ratio 0 when dk = 0), w = -expm1(-t / (2 / sd)^2);
    the row divided by its sum in that order (compensated_sum); a zero sum leaves a zero row"""
    pairs, score = np.asarray(pairs), np.asarray(score, dtype=np.float64)
    order = np.argsort(pairs[:, 1], kind="stable")                # anchors grouped by query cell, list order kept
    start = np.searchsorted(pairs[order, 1], np.arange(m + 1))
    den = (2.0 / float(sd_weight)) ** 2
    kw = WN.shape[1]
    rowptr, anchor, weight = [0], [], []
    for c in range(m):
        dk = float(WD[c, kw - 1])
        ids, ts = [], []
        for i in range(kw):
            ratio = float(WD[c, i]) / dk if dk > 0.0 else 0.0
            u = U[WN[c, i]]
            for a in order[start[u]:start[u + 1]]:
                ids.append(a)
                ts.append((1.0 - ratio) * score[a])
        w = -np.expm1(-np.array(ts, dtype=np.float64) / den)
        total = compensated_sum(w)
        anchor.append(np.array(ids, dtype=np.int32))
        weight.append(w / total if total > 0.0 else np.zeros(len(w)))
        rowptr.append(rowptr[-1] + len(ids))
    return np.array(rowptr, dtype=np.int64), np.concatenate(anchor), np.concatenate(weight)


def row_sums(rowptr, weight):
    """every row's sum, left to right"""
    out = np.zeros(len(rowptr) - 1)
    for c in range(len(out)):
        for e in range(rowptr[c], rowptr[c + 1]):
            out[c] += weight[e]
    return out


# ---- A6 -----------------------------------------------------------------------------------------------------------------------

def predict_labels(rowptr, anchor, weight, pairs, codes, L):
    """(label, score, scores): scores[c, l] = the row's weights over the anchors whose reference cell has code l, in row order;
    the largest wins, ties to the smaller code; -1 (score 0) where no class has a positive score"""
    m = len(rowptr) - 1
    scores = np.zeros((m, L))
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    code = np.asarray(codes)[np.asarray(pairs)[anchor, 0]]
    keep = code >= 0
    np.add.at(scores, (rows[keep], code[keep]), weight[keep])     # unbuffered: element by element, in order
    label = scores.argmax(axis=1).astype(np.int32)                # (the first maximum: the smaller code)
    score = scores[np.arange(m), label]
    label[~(score > 0.0)] = -1
    return label, np.where(score > 0.0, score, 0.0), scores


def predict_features(rowptr, anchor, weight, pairs, refdata):
    """fp64 (m, F): sum_a w_a * (double)refdata[r_a, f] over the row in row order, product and sum rounded apart; the device
    returns its float32"""
    ref = np.asarray(refdata, dtype=np.float32).astype(np.float64)
    m, lens = len(rowptr) - 1, np.diff(rowptr)
    acc = np.zeros((m, ref.shape[1]))
    for e in range(int(lens.max()) if m else 0):
        rows = np.flatnonzero(lens > e)
        at = rowptr[rows] + e
        acc[rows] = acc[rows] + weight[at][:, None] * ref[np.asarray(pairs)[anchor[at], 0]]
    return acc


def near_ties(scores, gap=1e-9):
    """the query cells whose two largest class scores differ by less than `gap` (with one class: none)"""
    if scores.shape[1] < 2:
        return np.zeros(len(scores), dtype=bool)
    top = np.sort(scores, axis=1)[:, -2:]
    return (top[:, 1] - top[:, 0]) < gap


# ---- the whole chain ------------------------------------------------------------------------------------------------------------

def find_anchors(X_query, X_ref, k_anchor=5, k_score=30, l2_norm=True):
    R, Q = np.asarray(X_ref, dtype=np.float32), np.asarray(X_query, dtype=np.float32)
    if l2_norm:
        R, Q = l2_normalize(R), l2_normalize(Q)
    K = max(k_anchor, k_score)
    if not 2 <= k_anchor <= K <= min(len(R), len(Q), 64):
        raise ValueError("need 2 <= k_anchor <= K <= min(n, m, 64)")
    RR, RQ, QR, QQ = knn_tables(R, Q, K)
    pairs = anchor_pairs(RQ, QR, k_anchor)
    raw = anchor_raw(pairs, RR, RQ, QR, QQ, k_score)
    return dict(R=R, Q=Q, RR=RR, RQ=RQ, QR=QR, QQ=QQ, pairs=pairs, raw=raw, score=normalize_scores(raw),
                U=anchor_queries(pairs))


def weights(found, k_weight=50, sd_weight=1.0):
    WN, WD = weight_knn(found["Q"], found["U"], k_weight)
    rowptr, anchor, weight = anchor_weights(found["pairs"], found["score"], len(found["Q"]), found["U"], WN, WD, sd_weight)
    return dict(WN=WN, WD=WD, rowptr=rowptr, anchor=anchor, weight=weight)
