"""Mapping held-out cells onto a clustered sample: exact kNN of new points against a reference set, and the transfer of the
reference's labels by a weighted neighbour vote.  The step the reference's sub-sampling flow ends with, in R:
`R/pbmc3k/Pbmc3k_data_subsampling_clusters.Rmd:34-44` (``colors_vec[!!pruned] <- colors2+2``: every cell that was not kept
stays at label 0) and Seurat's ``MapQuery`` (`Pbmc3k_assess_QA_clusters.Rmd:210-237`).  The embedding of the new points is
:func:`umap.transform`, built on the same handle.

Everything numeric past the argument checks runs in libmi_sa.so (csrc/mapping_kernels.hip, C ABI include/mi_umap.h); the
chain is specified in DESIGN.md section 5d ("chain Q").  A query's result depends on the reference and on that query alone,
never on which other queries are sent with it.

Anchor-based transfer (``FindTransferAnchors`` / ``TransferData``) is :mod:`anchors`.  Not built: the reference-range split
of the cross kNN (one wavefront serves 64 queries: few queries against a large reference leave most of the device idle).

    kept = np.flatnonzero([G.nodes[v]["label1"] for v in G.nodes])         # clustering.graph_subsampling
    ext = mapping.extend_labels(emb.coords[:, :15], kept, labels_kept)      # labels for all cells
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .preprocess import Result
from .umap import METRICS, _check_points

WEIGHTS = {"uniform": 0, "fuzzy": 1}


# ---- argument checks (all before any ctypes call) ---------------------------------------------------------------------------

def _check_pair(X_new, X_ref, k, metric):
    """the reference as :func:`umap._check_points` takes it, the queries against it"""
    R, k = _check_points(X_ref, k, metric)
    Q = np.asarray(X_new)
    if Q.ndim != 2 or Q.dtype.kind not in "fiu":
        raise ValueError("X_new must be a numeric (m, dim) array (got shape %s)" % (Q.shape,))
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    if Q.shape[0] < 1 or Q.shape[1] != R.shape[1]:
        raise ValueError("X_new must have m >= 1 rows of dim = %d (got shape %s)" % (R.shape[1], Q.shape))
    if not np.isfinite(Q).all():
        raise ValueError("X_new must be finite")
    return Q, R, k


def _check_labels(labels_ref, n):
    """-> (codes int32 with -1 for a negative label, classes): integer labels, coded through np.unique"""
    lab = np.asarray(labels_ref)
    if lab.shape != (n,) or lab.dtype.kind not in "iu":
        raise ValueError("labels_ref must be %d integers (negative: unlabelled)" % n)
    lab = lab.astype(np.int64)
    known = lab >= 0
    if not known.any():
        raise ValueError("labels_ref holds no label (every entry is negative)")
    classes, inv = np.unique(lab[known], return_inverse=True)
    codes = np.full(n, -1, dtype=np.int32)
    codes[known] = inv.astype(np.int32)
    return codes, classes


# ---- device passes -------------------------------------------------------------------------------------------------------------

class QueryGraph(_lib.Handle):
    """The ``mi_umap_query`` handle of include/mi_umap.h: Q1 (the cross kNN) on construction, then :meth:`smooth`,
    :meth:`vote` and :meth:`init`.  A context manager; ``timing`` collects the device milliseconds of every pass that has run."""
    _destroy = "mi_umap_query_destroy"

    def __init__(self, X_new, X_ref, n_neighbors: int, metric: str = "euclidean", device: int = 0):
        Q, R, k = _check_pair(X_new, X_ref, n_neighbors, metric)
        self.n, self.m, self.dim, self.k = R.shape[0], Q.shape[0], R.shape[1], k
        self.metric, self.device = metric, int(device)
        self.timing = {}
        h = C.c_void_p()
        self.timing["knn_ms"] = _lib.call_ms("mi_umap_query_knn_f32", R, self.n, Q, self.m, self.dim, k, METRICS[metric],
                                             self.device, h)
        self._h = h

    def fetch_knn(self):
        """``(nn, dist)``: m x k int32 indices into the reference by ascending (distance, index), m x k f32 distances."""
        nn = np.empty((self.m, self.k), dtype=np.int32)
        dist = np.empty((self.m, self.k), dtype=np.float32)
        _lib.call("mi_umap_query_fetch_knn", self._handle(), nn, dist)
        return nn, dist

    def smooth(self):
        self.timing["smooth_ms"] = _lib.call_ms("mi_umap_query_smooth", self._handle())
        return self

    def fetch_smooth(self):
        """``(sigma, weights)``: m fp64, m x k f32."""
        sigma = np.empty(self.m)
        w = np.empty((self.m, self.k), dtype=np.float32)
        _lib.call("mi_umap_query_fetch_smooth", self._handle(), sigma, w)
        return sigma, w

    def vote(self, codes, n_classes: int, weights: str = "fuzzy", return_scores: bool = False):
        """``(label, score[, scores])`` of chain Q5 on int32 ``codes`` (-1: unlabelled, else in ``[0, n_classes)``)."""
        h = self._handle()
        codes = np.asarray(codes)
        if weights not in WEIGHTS:
            raise ValueError("weights must be 'fuzzy' or 'uniform' (got %r)" % (weights,))
        if codes.shape != (self.n,) or codes.dtype != np.int32:
            raise ValueError("codes must be %d int32 values" % self.n)
        L = int(n_classes)
        if L < 1 or codes.min() < -1 or codes.max() >= L:
            raise ValueError("codes must be -1 or lie in [0, n_classes)")
        if return_scores and self.m * L >= 2 ** 31:
            raise ValueError("the dense score matrix would have m * n_classes = %d >= 2^31 cells" % (self.m * L))
        label = np.empty(self.m, dtype=np.int32)
        score = np.empty(self.m)
        scores = np.empty((self.m, L)) if return_scores else None
        self.timing["vote_ms"] = _lib.call_ms("mi_umap_query_vote", h, np.ascontiguousarray(codes), L, WEIGHTS[weights], label,
                                              score, scores)
        return (label, score, scores) if return_scores else (label, score)

    def init(self, Yref):
        """Chain Q3: the weighted mean of the neighbours' rows of ``Yref`` (n x 2 or n x 3), m x c f32."""
        h = self._handle()
        Yref = np.asarray(Yref)
        if Yref.ndim != 2 or Yref.shape[0] != self.n or Yref.shape[1] not in (2, 3) or Yref.dtype.kind not in "fiu":
            raise ValueError("Yref must be a numeric (%d, 2) or (%d, 3) array" % (self.n, self.n))
        Yref = np.ascontiguousarray(Yref, dtype=np.float32)
        if not np.isfinite(Yref).all():
            raise ValueError("Yref must be finite")
        Y0 = np.empty((self.m, Yref.shape[1]), dtype=np.float32)
        self.timing["init_ms"] = _lib.call_ms("mi_umap_query_init", h, Yref.shape[1], Yref, Y0)
        return Y0


def cross_knn(X_new, X_ref, k: int, metric: str = "euclidean", device: int = 0):
    """``(nn, dist)`` of chain Q1: for every row of ``X_new`` its ``k`` exact nearest rows of ``X_ref`` by ascending
    (distance, index) and their distances (``"cosine"``: 1 - cos).  Nothing is excluded: a row that also occurs in ``X_ref``
    finds it at distance 0."""
    with QueryGraph(X_new, X_ref, k, metric, device) as g:
        return g.fetch_knn()


def transfer_labels(X_new, X_ref, labels_ref, k: int = 30, metric: str = "euclidean", weights: str = "fuzzy",
                    return_scores: bool = False, device: int = 0) -> Result:
    """Labels for ``X_new`` by the vote of each row's ``k`` nearest rows of ``X_ref``.  ``labels_ref``: integers, a negative
    one means unlabelled (such neighbours do not vote).  ``weights="fuzzy"``: a neighbour counts its membership weight
    (umap-learn's transform rule); ``"uniform"``: every neighbour counts 1.  Ties go to the smaller label.  Returns
    ``labels`` (in the caller's values; -1 where no neighbour carries a label), ``score`` (the winner's share), ``nn``,
    ``dist``, ``timing`` and, with ``return_scores``, the dense ``scores`` (m x len(classes)) and ``classes``."""
    Q, R, k = _check_pair(X_new, X_ref, k, metric)
    if weights not in WEIGHTS:
        raise ValueError("weights must be 'fuzzy' or 'uniform' (got %r)" % (weights,))
    codes, classes = _check_labels(labels_ref, R.shape[0])
    if return_scores and Q.shape[0] * len(classes) >= 2 ** 31:
        raise ValueError("the dense score matrix would have %d >= 2^31 cells" % (Q.shape[0] * len(classes)))
    with QueryGraph(Q, R, k, metric, device) as g:
        nn, dist = g.fetch_knn()
        if weights == "fuzzy":
            g.smooth()
        out = g.vote(codes, len(classes), weights, return_scores)
        labels = np.where(out[0] >= 0, classes[np.maximum(out[0], 0)], -1)
        res = Result(labels=labels, score=out[1], nn=nn, dist=dist, timing=dict(g.timing))
        if return_scores:
            res["scores"], res["classes"] = out[2], classes
        return res


def extend_labels(X, kept, labels_kept, **kw) -> Result:
    """The last step of the sub-sampling flow: ``kept`` are the rows of ``X`` that were clustered (distinct indices),
    ``labels_kept`` their labels; every other row takes the label :func:`transfer_labels` gives it from the kept rows
    (keywords as there).  Returns ``labels`` and ``score`` for all rows of ``X`` (kept rows keep theirs, with score 1),
    ``held_out`` (the other rows' indices) and ``timing``."""
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError("X must be (n, dim) (got shape %s)" % (X.shape,))
    n = X.shape[0]
    kept = np.asarray(kept)
    if kept.ndim != 1 or kept.dtype.kind not in "iu" or len(kept) < 2:
        raise ValueError("kept must be a 1-d array of at least 2 row indices")
    kept = kept.astype(np.int64)
    if kept.min() < 0 or kept.max() >= n or len(np.unique(kept)) != len(kept):
        raise ValueError("kept must hold distinct indices in [0, %d)" % n)
    labels_kept = np.asarray(labels_kept)
    if labels_kept.shape != kept.shape or labels_kept.dtype.kind not in "iu":
        raise ValueError("labels_kept must be one integer per kept row")
    if kw.get("return_scores"):
        raise ValueError("extend_labels returns no score matrix: call transfer_labels for one")
    mask = np.ones(n, dtype=bool)
    mask[kept] = False
    held = np.flatnonzero(mask)
    labels = np.empty(n, dtype=np.int64)
    score = np.ones(n)
    labels[kept] = labels_kept
    timing = {}
    if len(held):
        res = transfer_labels(X[held], X[kept], labels_kept, **kw)
        labels[held], score[held], timing = res.labels, res.score, res.timing
    return Result(labels=labels, score=score, held_out=held, timing=timing)
