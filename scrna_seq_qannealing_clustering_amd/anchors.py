"""Anchor-based label and feature transfer: Seurat v4's ``FindTransferAnchors`` followed by ``TransferData`` / ``MapQuery``,
the step the reference's assessment notebook ends with (`R/pbmc3k/Pbmc3k_assess_QA_clusters.Rmd:210-237`:
``MapQuery(..., refdata = list(celltype.l1, celltype.l2, predicted_ADT = "ADT"))``): an annotated reference's cell types and
measured proteins carried over to the query cells through mutual nearest neighbours ("anchors"), each scored by the
neighbourhoods the two cells share and weighted per query cell by distance.

Everything numeric past the argument checks, the row normalisation's specification and the quantile rescaling of the scores
runs in libmi_sa.so (csrc/anchor_kernels.hip, C ABI include/mi_anchors.h); the chain is specified in DESIGN.md section 5d
("chain A") and restated in numpy by tests/anchor_reference.py.  This is this package's specification, modelled on Seurat's
``FindAnchorPairs``, ``ScoreAnchors``, ``FindWeights`` and ``TransferData``; agreement with R is unpinned.  Unlike chain Q
(:mod:`mapping`), a query cell's result depends on the other query cells of the call: they are each other's neighbours.

Both point sets must lie in one common space: the PCA coordinates of :func:`preprocess.embed` / ``sctransform`` on the cells
together, or ``X[kept]`` / ``X[held_out]`` of the sub-sampling flow.

Not built: ``k.filter`` (it needs k = 200 > 64 neighbours in feature space), projecting a query onto a reference's stored PCA
loadings, ``IntegrateEmbeddings``, ``MappingScore``, ``reduction = "cca"`` / ``"rpca"``.

    with anchors.find_transfer_anchors(X_query, X_ref) as aset:
        out = anchors.transfer_data(aset, {"celltype": labels_ref, "ADT": adt_ref})
    out["celltype"].labels, out["ADT"].predicted
"""
from __future__ import annotations

import ctypes as C
import math
import time

import numpy as np

from . import _lib
from .mapping import _check_labels
from .preprocess import Result

MAX_K = 64
PASSES = ("knn_ms", "pairs_ms", "score_ms", "weight_knn_ms", "weights_ms")


# ---- argument checks (all before any ctypes call) ---------------------------------------------------------------------------

def _check_int(value, name, lo):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < lo:
        raise ValueError("%s must be an integer >= %d (got %r)" % (name, lo, value))
    return int(value)


def _check_points(X, name):
    X = np.asarray(X)
    if X.ndim != 2 or X.dtype.kind not in "fiu":
        raise ValueError("%s must be a numeric (cells, dim) array (got shape %s)" % (name, X.shape))
    X = np.ascontiguousarray(X, dtype=np.float32)
    if not np.isfinite(X).all():
        raise ValueError("%s must be finite" % name)
    return X


def _check_sets(X_query, X_ref, k_anchor, k_score, l2_norm):
    """-> (Q, R, k_anchor, k_score) as mi_anchors_find_f32 takes them"""
    R, Q = _check_points(X_ref, "X_ref"), _check_points(X_query, "X_query")
    n, dim = R.shape
    m = Q.shape[0]
    if not 1 <= dim <= 64:
        raise ValueError("need 1 <= dim <= 64 (got %d)" % dim)
    if Q.shape[1] != dim:
        raise ValueError("X_query must have dim = %d columns, as X_ref (got shape %s)" % (dim, Q.shape))
    ka, ks = _check_int(k_anchor, "k_anchor", 2), _check_int(k_score, "k_score", 1)
    K = max(ka, ks)
    if K > min(n, m, MAX_K):
        raise ValueError("need max(k_anchor, k_score) <= min(n, m, 64) (got k_anchor=%d k_score=%d n=%d m=%d)" % (ka, ks, n, m))
    if l2_norm not in (True, False):
        raise ValueError("l2_norm must be True or False (got %r)" % (l2_norm,))
    if l2_norm:
        for name, X in (("X_ref", R), ("X_query", Q)):
            zero = np.flatnonzero(~X.any(axis=1))
            if len(zero):
                raise ValueError("row %d of %s is all zero: l2_norm cannot give it a direction" % (zero[0], name))
    return Q, R, ka, ks


def _check_weight_args(k_weight, sd_weight):
    kw = _check_int(k_weight, "k_weight", 2)
    if kw > MAX_K:
        raise ValueError("need k_weight <= 64 (got %d)" % kw)
    if isinstance(sd_weight, bool) or not isinstance(sd_weight, (int, float, np.integer, np.floating)) \
            or not math.isfinite(sd_weight) or not sd_weight > 0:
        raise ValueError("sd_weight must be a finite number > 0 (got %r)" % (sd_weight,))
    return kw, float(sd_weight)


def _check_k_weight(k_weight: int, n_anchor_queries: int):
    """Seurat stops here too: the weights of a query cell are taken over its ``k_weight`` nearest anchor query cells"""
    if k_weight > n_anchor_queries:
        raise ValueError("k_weight = %d exceeds |U| = %d, the number of distinct query cells with an anchor"
                         % (k_weight, n_anchor_queries))


def _check_refdata(refdata, n: int, m: int):
    """one item of refdata -> ("labels", codes, classes) | ("features", (n, F) f32)"""
    arr = np.asarray(refdata)
    if arr.shape == (n,) and arr.dtype.kind in "iu":
        codes, classes = _check_labels(arr, n)
        return "labels", codes, classes
    if arr.ndim == 2 and arr.dtype.kind in "fiu" and arr.shape[0] == n and arr.shape[1] >= 1:
        if m * arr.shape[1] >= 2 ** 31:
            raise ValueError("the prediction would have m * F = %d >= 2^31 cells" % (m * arr.shape[1]))
        arr = np.ascontiguousarray(arr, dtype=np.float32)
        if not np.isfinite(arr).all():
            raise ValueError("refdata must be finite")
        return "features", arr, None
    raise ValueError("refdata must be %d integer labels (negative: unlabelled), a numeric (%d, F) array or a dict of such "
                     "(got shape %s, dtype %s)" % (n, n, arr.shape, arr.dtype))


def _check_refdata_arg(refdata, n: int, m: int, return_scores: bool):
    """-> (items as {name: checked}, whether the caller passed a dict)"""
    if isinstance(refdata, dict):
        if not refdata:
            raise ValueError("refdata is an empty dict")
        items = {name: _check_refdata(v, n, m) for name, v in refdata.items()}
    else:
        items = {None: _check_refdata(refdata, n, m)}
    for kind, _, classes in items.values():
        if kind == "labels" and return_scores and m * len(classes) >= 2 ** 31:
            raise ValueError("the dense score matrix would have %d >= 2^31 cells" % (m * len(classes)))
    return items, isinstance(refdata, dict)


def normalize_scores(raw) -> np.ndarray:
    """Chain A3's host half: ``clip((raw - lo) / (hi - lo), 0, 1)`` with ``lo, hi = np.quantile(raw, [0.01, 0.90])`` in fp64
    (Seurat's ``ScoreAnchors``).  If ``hi == lo`` every score is 1: Seurat divides by zero there."""
    raw = np.asarray(raw, dtype=np.float64)
    if raw.size == 0:
        return np.zeros(0)
    lo, hi = np.quantile(raw, [0.01, 0.90])
    if hi == lo:
        return np.ones(raw.shape)
    return np.clip((raw - lo) / (hi - lo), 0.0, 1.0)


# ---- device passes -------------------------------------------------------------------------------------------------------------

class AnchorSet(_lib.Handle):
    """The ``mi_anchors`` handle of include/mi_anchors.h: chain A0 - A3 on construction (the four kNN tables, the anchors and
    their scores stay on the device), then :meth:`weights` (A4 - A5) and the predictions (A6).  A context manager.
    ``anchors``: (A, 2) int32 (reference cell, query cell) by ascending reference cell, then by the query cell's rank among
    that cell's neighbours; ``raw_score``: the shared-neighbour counts; ``score``: in [0, 1]; ``timing``: device ms per pass."""
    _destroy = "mi_anchors_destroy"

    def __init__(self, X_query, X_ref, k_anchor: int = 5, k_score: int = 30, l2_norm: bool = True, device: int = 0):
        Q, R, ka, ks = _check_sets(X_query, X_ref, k_anchor, k_score, l2_norm)
        self.n, self.m, self.dim = R.shape[0], Q.shape[0], R.shape[1]
        self.k_anchor, self.k_score, self.K, self.l2_norm, self.device = ka, ks, max(ka, ks), bool(l2_norm), int(device)
        self.timing = {}
        self._weights_key = None
        h = C.c_void_p()
        _lib.call_ms("mi_anchors_find_f32", R, self.n, Q, self.m, self.dim, ka, ks, int(self.l2_norm), self.device, h)
        self._h = h
        info = self.info()
        A = info["n_anchors"]
        self.anchors = np.empty((A, 2), dtype=np.int32)
        self.raw_score = np.empty(A, dtype=np.int32)
        _lib.call("mi_anchors_fetch", h, self.anchors, self.raw_score, None, None, None, None)
        self.score = normalize_scores(self.raw_score)
        _lib.call("mi_anchors_set_scores", h, self.score)
        self.n_anchor_queries = info["n_anchor_queries"]

    def info(self) -> dict:
        A, U, nnz, nbytes = C.c_int(0), C.c_int(0), C.c_int64(0), C.c_int64(0)
        ms = np.zeros(len(PASSES), dtype=np.float32)
        _lib.call("mi_anchors_info", self._handle(), A, U, nnz, nbytes, ms)
        self.timing.update({name: float(v) for name, v in zip(PASSES, ms) if v > 0.0 or name in self.timing})
        return dict(n_anchors=int(A.value), n_anchor_queries=int(U.value), nnz=int(nnz.value), device_bytes=int(nbytes.value))

    def device_bytes(self) -> int:
        """bytes the handle holds on the device now; 0 once it is closed"""
        if self._h is None or not self._h.value:
            return 0
        return self.info()["device_bytes"]

    def fetch_tables(self):
        """``(RR, RQ, QR, QQ)`` of chain A1: n x K reference-in-reference and reference-in-query, m x K query-in-reference and
        query-in-query neighbours by ascending (distance, index); a cell is its own first neighbour in RR and QQ."""
        h = self._handle()
        RR, RQ = (np.empty((self.n, self.K), dtype=np.int32) for _ in range(2))
        QR, QQ = (np.empty((self.m, self.K), dtype=np.int32) for _ in range(2))
        _lib.call("mi_anchors_fetch", h, None, None, RR, RQ, QR, QQ)
        return RR, RQ, QR, QQ

    def _ensure_weights(self, k_weight, sd_weight):
        h = self._handle()
        kw, sd = _check_weight_args(k_weight, sd_weight)
        _check_k_weight(kw, self.n_anchor_queries)
        if self._weights_key != (kw, sd):
            self._weights_key = None
            _lib.call_ms("mi_anchors_weights", h, kw, sd)
            self._weights_key = (kw, sd)
            self.info()
        return kw

    def weights(self, k_weight: int = 50, sd_weight: float = 1.0) -> Result:
        """Chain A4 - A5: for every query cell the weights of the anchors of its ``k_weight`` nearest anchor query cells, as
        a CSR over the query cells: ``rowptr`` (m + 1), ``anchor`` (indices into ``anchors``), ``weight`` (fp64; a row sums
        to 1 or is all zero), and the neighbours ``wn`` (indices into the sorted distinct anchor query cells) / ``wd``."""
        kw = self._ensure_weights(k_weight, sd_weight)
        nnz = self.info()["nnz"]
        rowptr = np.empty(self.m + 1, dtype=np.int64)
        anchor, weight = np.empty(nnz, dtype=np.int32), np.empty(nnz)
        wn, wd = np.empty((self.m, kw), dtype=np.int32), np.empty((self.m, kw), dtype=np.float32)
        _lib.call("mi_anchors_fetch_weights", self._handle(), rowptr, anchor, weight, wn, wd)
        return Result(rowptr=rowptr, anchor=anchor, weight=weight, wn=wn, wd=wd)

    def predict_labels(self, codes, n_classes: int, return_scores: bool = False):
        """``(label, score[, scores])`` of chain A6 on int32 ``codes`` (-1: unlabelled, else in ``[0, n_classes)``), on the
        weights computed last."""
        h = self._handle()
        if self._weights_key is None:
            raise ValueError("predict_labels before weights()")
        codes = np.asarray(codes)
        if codes.shape != (self.n,) or codes.dtype != np.int32:
            raise ValueError("codes must be %d int32 values" % self.n)
        L = int(n_classes)
        if L < 1 or codes.min() < -1 or codes.max() >= L:
            raise ValueError("codes must be -1 or lie in [0, n_classes)")
        if return_scores and self.m * L >= 2 ** 31:
            raise ValueError("the dense score matrix would have m * n_classes = %d >= 2^31 cells" % (self.m * L))
        label, score = np.empty(self.m, dtype=np.int32), np.empty(self.m)
        scores = np.empty((self.m, L)) if return_scores else None
        self.timing["predict_labels_ms"] = _lib.call_ms("mi_anchors_predict_labels", h, np.ascontiguousarray(codes), L, label,
                                                        score, scores)
        return (label, score, scores) if return_scores else (label, score)

    def predict_features(self, refdata):
        """Chain A6 on an (n, F) array: the (m, F) f32 weighted sums, on the weights computed last."""
        h = self._handle()
        if self._weights_key is None:
            raise ValueError("predict_features before weights()")
        kind, ref, _ = _check_refdata(refdata, self.n, self.m)
        if kind != "features":
            raise ValueError("refdata must be a numeric (%d, F) array" % self.n)
        pred = np.empty((self.m, ref.shape[1]), dtype=np.float32)
        self.timing["predict_features_ms"] = _lib.call_ms("mi_anchors_predict_features", h, ref, ref.shape[1], pred)
        return pred


def find_transfer_anchors(X_query, X_ref, k_anchor: int = 5, k_score: int = 30, l2_norm: bool = True,
                          device: int = 0) -> AnchorSet:
    """Seurat's ``FindTransferAnchors`` on two point sets in one common space (its ``k.anchor``, ``k.score``, ``l2.norm``
    with their defaults; no ``k.filter``): the open :class:`AnchorSet`.  Use it in a ``with`` block."""
    return AnchorSet(X_query, X_ref, k_anchor, k_score, l2_norm, device)


def _transfer(aset, items, as_dict, return_scores):
    out = {}
    for name, (kind, data, classes) in items.items():
        if kind == "labels":
            got = aset.predict_labels(data, len(classes), return_scores)
            res = Result(labels=np.where(got[0] >= 0, classes[np.maximum(got[0], 0)], -1), score=got[1])
            if return_scores:
                res["scores"], res["classes"] = got[2], classes
        else:
            res = Result(predicted=aset.predict_features(data))
        res["timing"] = dict(aset.timing)
        out[name] = res
    return out if as_dict else out[None]


def transfer_data(anchorset: AnchorSet, refdata, k_weight: int = 50, sd_weight: float = 1.0, return_scores: bool = False):
    """Seurat's ``TransferData``.  ``refdata``: ``n`` integer labels of the reference cells (any values; a negative one means
    unlabelled), a numeric (n, F) array (such as the ADT matrix), or a dict of such (Seurat's ``refdata = list(...)``), which
    returns a dict of results from ONE weights pass.  Labels give ``labels`` (the caller's values; -1 where no class has a
    positive score), ``score`` (the winner's: ``prediction.score.max``) and, with ``return_scores``, the dense ``scores``
    (m x len(classes)) and ``classes``; ties go to the smaller label.  Features give ``predicted`` (m, F) f32."""
    if not isinstance(anchorset, AnchorSet):
        raise ValueError("anchorset must be an AnchorSet (find_transfer_anchors)")
    anchorset._handle()
    kw, _ = _check_weight_args(k_weight, sd_weight)
    _check_k_weight(kw, anchorset.n_anchor_queries)
    items, as_dict = _check_refdata_arg(refdata, anchorset.n, anchorset.m, return_scores)
    anchorset._ensure_weights(k_weight, sd_weight)
    return _transfer(anchorset, items, as_dict, return_scores)


def map_query(X_query, X_ref, refdata, um=None, k_anchor: int = 5, k_score: int = 30, l2_norm: bool = True,
              k_weight: int = 50, sd_weight: float = 1.0, return_scores: bool = False, device: int = 0, umap_kw=None) -> Result:
    """The reference's ``FindTransferAnchors`` + ``MapQuery`` call in one line: anchors, then :func:`transfer_data`, then,
    when ``um`` (the :func:`umap.run_umap` result fitted on ``X_ref``) is given, :func:`umap.transform` with ``umap_kw``
    (pass the fit's ``n_neighbors`` and ``metric``).  Returns ``transfer`` (what :func:`transfer_data` returns), ``anchors``,
    ``anchor_score``, ``timing`` and, with ``um``, ``coords`` and ``umap`` (the transform's result)."""
    t_all = time.perf_counter()
    Q, R, ka, ks = _check_sets(X_query, X_ref, k_anchor, k_score, l2_norm)
    _check_weight_args(k_weight, sd_weight)
    _check_refdata_arg(refdata, R.shape[0], Q.shape[0], return_scores)
    if umap_kw is not None and (um is None or not isinstance(umap_kw, dict)):
        raise ValueError("umap_kw is a dict of umap.transform's keywords and needs um")
    with AnchorSet(Q, R, ka, ks, l2_norm, device) as aset:
        transfer = transfer_data(aset, refdata, k_weight, sd_weight, return_scores)
        res = Result(transfer=transfer, anchors=aset.anchors, anchor_score=aset.score, timing=dict(aset.timing))
    if um is not None:
        from . import umap
        placed = umap.transform(Q, R, um, device=device, **(umap_kw or {}))
        res["coords"], res["umap"] = placed.coords, placed
    res["timing"]["total_ms"] = (time.perf_counter() - t_all) * 1e3
    return res
