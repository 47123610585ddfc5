"""UMAP on the GPU: points -> exact kNN with distances -> smooth kNN distances -> fuzzy union graph -> a deterministic SGD
layout.  The picture every notebook of the reference ends with, in R (Seurat):
`R/pbmc3k/Pbmc3k_assess_QA_clusters.Rmd:94-108`, `R/kidney/Kidney_data.Rmd:133-155,183`, `Kidney_subsampling.Rmd:47,86`:
``RunUMAP(obj, dims = 1:15)`` then ``DimPlot(reduction = "umap", group.by = ...)``.

Everything numeric past the argument checks runs in libmi_sa.so (csrc/umap_kernels.hip, C ABI include/mi_umap.h); the curve
constants ``a, b`` and the initial coordinates are host fp64.  The chain is specified in DESIGN.md section 5d: every epoch
of the layout is a gather from the previous epoch's positions with counter-based negatives, so two calls return
bit-identical coordinates (umap-learn's and uwot's layouts are racy loops: theirs do not).

Not built: spectral initialisation (``init="pca"`` or an array), supervised UMAP, metrics other than ``"euclidean"`` and
``"cosine"``.

    emb = preprocess.embed(counts, nfeatures=2000, npcs=50)
    um = umap.run_umap(emb.coords[:, :15])            # Seurat's RunUMAP(dims = 1:15) defaults
    outputs.plot_and_save_embedding(um.coords, labels, "umap.png")

New points are placed in a fitted embedding by :func:`transform` (chain Q of DESIGN.md section 5d, csrc/mapping_kernels.hip):
the reference embedding stays fixed, every query runs all its epochs in registers in one launch, and a query's coordinates
do not depend on which other queries are sent with it.

    um = umap.run_umap(X[kept])
    rest = umap.transform(X[held_out], X[kept], um)    # .coords: where the held-out cells fall in um.coords' picture
"""
from __future__ import annotations

import ctypes as C
import math
import time

import numpy as np

from . import _lib
from .preprocess import Result

METRICS = {"euclidean": 0, "cosine": 1}                      # MI_UMAP_EUCLIDEAN, MI_UMAP_COSINE
MAX_EPOCHS = 10000                                           # MI_UMAP_MAX_EPOCHS
MAX_NEGATIVE = 16                                            # MI_UMAP_MAX_NEGATIVE

class UmapResult(Result):
    """``coords`` (n x c f32), ``nn``, ``dist``, ``rho``, ``sigma``, the fuzzy graph as ``rowptr`` / ``col`` / ``weights``,
    ``a``, ``b``, ``n_epochs`` and ``timing`` (kernel ms per stage, host ms)."""


# ---- host side, fp64 ----------------------------------------------------------------------------------------------------------

def find_ab_params(spread: float = 1.0, min_dist: float = 0.3):
    """``(a, b)`` of the curve ``1 / (1 + a x^(2b))``: least squares to umap's target (1 for ``x < min_dist``, else
    ``exp(-(x - min_dist) / spread)``) on 300 points of ``[0, 3 spread]``, by Levenberg-Marquardt from ``(1, 1)`` in numpy
    fp64 (umap-learn calls scipy's ``curve_fit`` for the same problem)."""
    spread, min_dist = float(spread), float(min_dist)
    if not (math.isfinite(spread) and spread > 0.0):
        raise ValueError("spread must be finite and > 0")
    if not (math.isfinite(min_dist) and 0.0 <= min_dist <= spread):
        raise ValueError("min_dist must lie in [0, spread]")
    x = np.linspace(0.0, 3.0 * spread, 300)
    y = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))
    lnx = np.log(np.where(x > 0.0, x, 1.0))

    def model(p):
        u = np.where(x > 0.0, np.exp(2.0 * p[1] * lnx), 0.0)
        f = 1.0 / (1.0 + p[0] * u)
        J = np.stack([-u * f * f, -2.0 * p[0] * u * lnx * f * f], axis=1)
        return f, J

    p = np.array([1.0, 1.0])
    f, J = model(p)
    sse, lam = float(((y - f) ** 2).sum()), 1e-3
    for _ in range(500):
        A, g = J.T @ J, J.T @ (y - f)
        step = np.linalg.solve(A + lam * np.diag(np.diag(A)), g)
        q = p + step
        if q[0] > 0.0 and q[1] > 0.0:
            fq, Jq = model(q)
            sq = float(((y - fq) ** 2).sum())
        else:
            sq = math.inf
        if sq < sse:
            done = np.abs(step).max() < 1e-13 * np.abs(p).max()
            p, f, J, sse, lam = q, fq, Jq, sq, lam / 10.0
            if done:
                break
        else:
            lam *= 10.0
            if lam > 1e12:
                break
    return float(p[0]), float(p[1])


def pca_init(X, n_components: int = 2) -> np.ndarray:
    """The first ``n_components`` columns of ``X``, centred, scaled by one common factor so that the largest absolute
    coordinate is 10 (all zeros stay zeros); fp64 arithmetic, f32 result."""
    X = np.asarray(X)
    c = int(n_components)
    if c not in (2, 3):
        raise ValueError("n_components must be 2 or 3 (got %d)" % c)
    if X.ndim != 2 or X.shape[1] < c:
        raise ValueError("init='pca' takes the first %d columns of X: X has shape %s" % (c, X.shape))
    Y = X[:, :c].astype(np.float64)
    if not np.isfinite(Y).all():
        raise ValueError("X must be finite")
    Y = Y - Y.mean(axis=0)
    top = np.abs(Y).max() if Y.size else 0.0
    if top > 0.0:
        Y = Y * (10.0 / top)
    return np.ascontiguousarray(Y, dtype=np.float32)


def default_n_epochs(n: int) -> int:
    """umap-learn's and uwot's rule: 500 epochs up to 10 000 points, 200 above."""
    return 500 if int(n) <= 10000 else 200


def normalize_rows(X) -> np.ndarray:
    """What ``metric="cosine"`` searches: every row divided by its norm (fp64 sum of squares in coordinate order, sqrt, fp64
    quotient rounded to f32; an all-zero row stays zero) -- the host step of include/mi_umap.h, restated."""
    X64 = np.ascontiguousarray(X, dtype=np.float32).astype(np.float64)
    ss = np.zeros(X64.shape[0])
    for c in range(X64.shape[1]):
        ss = ss + X64[:, c] * X64[:, c]
    nrm = np.sqrt(ss)
    out = np.zeros_like(X64)
    ok = nrm > 0.0
    out[ok] = X64[ok] / nrm[ok, None]
    return out.astype(np.float32)


# ---- argument checks (all before any ctypes call) ---------------------------------------------------------------------------

def _check_points(X, k, metric):
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError("X must be (n, dim) (got shape %s)" % (X.shape,))
    if X.dtype.kind not in "fiu":
        raise ValueError("X must be numeric")
    X = np.ascontiguousarray(X, dtype=np.float32)
    n, dim = X.shape
    if not 1 <= dim <= 64:
        raise ValueError("need 1 <= dim <= 64 (got %d)" % dim)
    if isinstance(k, bool) or int(k) != k:
        raise ValueError("n_neighbors must be an integer")
    k = int(k)
    if n < 2 or k < 2 or k > 64 or k > n:
        raise ValueError("need n >= 2 and 2 <= n_neighbors <= min(64, n) (got n=%d n_neighbors=%d)" % (n, k))
    if metric not in METRICS:
        raise ValueError("metric must be 'euclidean' or 'cosine' (got %r)" % (metric,))
    if not np.isfinite(X).all():
        raise ValueError("X must be finite")
    return X, k


def _check_layout_args(n_epochs, learning_rate, negative_sample_rate, seed):
    if isinstance(n_epochs, bool) or int(n_epochs) != n_epochs or not 1 <= int(n_epochs) <= MAX_EPOCHS:
        raise ValueError("n_epochs must be an integer in [1, %d] (got %r)" % (MAX_EPOCHS, n_epochs))
    neg = negative_sample_rate
    if isinstance(neg, bool) or int(neg) != neg or not 0 <= int(neg) <= MAX_NEGATIVE:
        raise ValueError("negative_sample_rate must be an integer in [0, %d] (got %r)" % (MAX_NEGATIVE, neg))
    lr = float(learning_rate)
    if not (math.isfinite(lr) and lr > 0.0):
        raise ValueError("learning_rate must be finite and > 0")
    if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
        raise ValueError("seed must be an integer in [0, 2^64)")
    return int(n_epochs), lr, int(neg), int(seed)


def _check_init(init, X, n, c):
    if isinstance(init, str):
        if init != "pca":
            raise ValueError("init must be 'pca' or an (n, n_components) array (spectral initialisation is not built)")
        if X is None:
            raise ValueError("init='pca' needs the points")
        return pca_init(X, c)
    Y0 = np.asarray(init)
    if Y0.dtype.kind not in "fiu" or Y0.shape != (n, c):
        raise ValueError("init must be 'pca' or a numeric array of shape (%d, %d)" % (n, c))
    Y0 = np.ascontiguousarray(Y0, dtype=np.float32)
    if not np.isfinite(Y0).all():
        raise ValueError("init must be finite")
    return Y0


# ---- device passes -------------------------------------------------------------------------------------------------------------

class FuzzyGraph(_lib.Handle):
    """The handle of include/mi_umap.h: U1 on construction, then :meth:`smooth` and :meth:`union`.  A context manager;
    ``timing`` collects the device milliseconds of every pass that has run."""
    _destroy = "mi_umap_destroy"

    def __init__(self, X, n_neighbors: int, metric: str = "euclidean", device: int = 0):
        X, k = _check_points(X, n_neighbors, metric)
        self.n, self.dim, self.k = X.shape[0], X.shape[1], k
        self.metric, self.device = metric, int(device)
        self.timing = {}
        h = C.c_void_p()
        self.timing["knn_ms"] = _lib.call_ms("mi_umap_knn_f32", X, self.n, self.dim, k, METRICS[metric], self.device, h)
        self._h = h

    def fetch_knn(self):
        """``(nn, dist)``: n x k int32 indices as :func:`snn.build_snn` returns them, n x k f32 distances."""
        nn = np.empty((self.n, self.k), dtype=np.int32)
        dist = np.empty((self.n, self.k), dtype=np.float32)
        _lib.call("mi_umap_fetch_knn", self._handle(), nn, dist)
        return nn, dist

    def smooth(self):
        self.timing["smooth_ms"] = _lib.call_ms("mi_umap_smooth", self._handle())
        return self

    def fetch_smooth(self):
        """``(rho, sigma)``, fp64."""
        rho, sigma = np.empty(self.n), np.empty(self.n)
        _lib.call("mi_umap_fetch_smooth", self._handle(), rho, sigma)
        return rho, sigma

    def union(self):
        self.timing["union_ms"] = _lib.call_ms("mi_umap_union", self._handle())
        return self

    def info(self) -> dict:
        nnz, deg, wmax = C.c_int64(0), C.c_int(0), C.c_float(0.0)
        _lib.call("mi_umap_info", self._handle(), None, None, nnz, deg, wmax)
        return {"nnz": int(nnz.value), "max_degree": int(deg.value), "w_max": float(wmax.value)}

    def fetch_graph(self):
        """``(rowptr, col, weights)``: the symmetric CSR (int64, int32, f32), rows ascending by column."""
        rowptr = np.empty(self.n + 1, dtype=np.int64)
        _lib.call("mi_umap_fetch_graph", self._handle(), rowptr, None, None)
        col = np.empty(int(rowptr[-1]), dtype=np.int32)
        w = np.empty(int(rowptr[-1]), dtype=np.float32)
        _lib.call("mi_umap_fetch_graph", self._handle(), None, col, w)
        return rowptr, col, w


def knn(X, k: int, metric: str = "euclidean", device: int = 0):
    """``(nn, dist)`` of chain U1: exact neighbours (column 0 the point itself) and their distances; ``"cosine"``: 1 - cos."""
    with FuzzyGraph(X, k, metric, device) as g:
        return g.fetch_knn()


def fuzzy_graph(X, k: int, metric: str = "euclidean", device: int = 0) -> Result:
    """Chain U1 - U3: ``nn``, ``dist``, ``rho``, ``sigma``, ``rowptr``, ``col``, ``weights``, ``max_degree``, ``w_max``,
    ``timing``."""
    with FuzzyGraph(X, k, metric, device) as g:
        nn, dist = g.fetch_knn()
        rho, sigma = g.smooth().fetch_smooth()
        rowptr, col, w = g.union().fetch_graph()
        info = g.info()
        return Result(nn=nn, dist=dist, rho=rho, sigma=sigma, rowptr=rowptr, col=col, weights=w,
                      max_degree=info["max_degree"], w_max=info["w_max"], timing=dict(g.timing))


def layout(rowptr, col, w, init, a: float, b: float, n_epochs: int = 500, learning_rate: float = 1.0,
           negative_sample_rate: int = 5, seed: int = 42, device: int = 0, return_ms: bool = False):
    """Chain U4 on any symmetric CSR (e.g. ``g.rowptr, g.col, g.weights`` of :func:`snn.build_snn`): ``init`` is the
    (n, 2) or (n, 3) start; returns the coordinates after ``n_epochs`` epochs (and the kernels' ms with ``return_ms``).
    What is wrong with the graph itself (unsorted or out-of-range columns, a diagonal entry, a weight that is not finite
    and positive) is reported by the library."""
    rowptr = np.asarray(rowptr)
    col, w = np.asarray(col), np.asarray(w)
    if rowptr.ndim != 1 or len(rowptr) < 2 or rowptr.dtype.kind not in "iu":
        raise ValueError("rowptr must be a 1-d integer array of n + 1 entries")
    n = len(rowptr) - 1
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
    if col.ndim != 1 or col.dtype.kind not in "iu" or w.ndim != 1 or w.dtype.kind not in "fiu":
        raise ValueError("col must be a 1-d integer array and w a 1-d numeric array")
    if len(col) != rowptr[-1] or len(w) != rowptr[-1]:
        raise ValueError("col and w must have rowptr[-1] = %d entries" % rowptr[-1])
    if len(col) and (col.min() < -2 ** 31 or col.max() >= 2 ** 31):
        raise ValueError("column index out of range")
    col = np.ascontiguousarray(col, dtype=np.int32)
    w = np.ascontiguousarray(w, dtype=np.float32)
    Y0 = np.asarray(init)
    if Y0.ndim != 2 or Y0.shape[0] != n or Y0.dtype.kind not in "fiu":
        raise ValueError("init must be a numeric (n, n_components) array with n = %d" % n)
    Y0 = np.ascontiguousarray(Y0, dtype=np.float32)
    a, b = float(a), float(b)
    if not (math.isfinite(a) and math.isfinite(b)):
        raise ValueError("a and b must be finite")
    T, lr, neg, seed = _check_layout_args(n_epochs, learning_rate, negative_sample_rate, seed)
    out = np.empty_like(Y0)
    ms = _lib.call_ms("mi_umap_layout_f32", n, Y0.shape[1], rowptr, col, w, Y0, a, b, lr, T, neg, C.c_uint64(seed), int(device),
                      out)
    return (out, ms) if return_ms else out


def run_umap(X, n_neighbors: int = 30, n_components: int = 2, metric: str = "cosine", min_dist: float = 0.3,
             spread: float = 1.0, n_epochs=None, learning_rate: float = 1.0, negative_sample_rate: int = 5, init="pca",
             seed: int = 42, device: int = 0) -> UmapResult:
    """Seurat's ``RunUMAP`` with its defaults (``n.neighbors = 30``, ``metric = "cosine"``, ``min.dist = 0.3``, ...), on
    ``X`` = the PCA coordinates (``emb.coords[:, :15]`` for ``dims = 1:15``).  ``init``: ``"pca"`` (the first columns of
    ``X``, see :func:`pca_init`) or an (n, n_components) array; spectral initialisation is not built.  ``n_epochs=None``:
    500 up to 10 000 points, else 200.  Two calls with the same arguments return bit-identical coordinates."""
    t_all = time.perf_counter()
    X, k = _check_points(X, n_neighbors, metric)
    n = X.shape[0]
    if isinstance(n_components, bool) or n_components not in (2, 3):
        raise ValueError("n_components must be 2 or 3 (got %r)" % (n_components,))
    c = int(n_components)
    T, lr, neg, seed = _check_layout_args(default_n_epochs(n) if n_epochs is None else n_epochs, learning_rate,
                                          negative_sample_rate, seed)
    a, b = find_ab_params(spread, min_dist)
    Y0 = _check_init(init, X, n, c)
    fg = fuzzy_graph(X, k, metric, device)
    a32, b32 = float(np.float32(a)), float(np.float32(b))
    coords, ms = layout(fg.rowptr, fg.col, fg.weights, Y0, a32, b32, T, lr, neg, seed, device, return_ms=True)
    timing = dict(fg.timing)
    timing["layout_ms"] = ms
    timing["epoch_ms"] = ms / T
    total_ms = (time.perf_counter() - t_all) * 1e3
    timing["host_ms"] = total_ms - sum(timing[s] for s in ("knn_ms", "smooth_ms", "union_ms", "layout_ms"))
    timing["total_ms"] = total_ms
    return UmapResult(coords=coords, nn=fg.nn, dist=fg.dist, rho=fg.rho, sigma=fg.sigma, rowptr=fg.rowptr, col=fg.col,
                      weights=fg.weights, a=a32, b=b32, n_epochs=T, timing=timing)


# ---- new points in a fitted embedding (chain Q) ---------------------------------------------------------------------------------

def transform_layout(nn, w, Yref, init, a: float, b: float, alpha0: float, n_epochs: int, negative_sample_rate: int = 5,
                     seed: int = 42, first_index: int = 0, device: int = 0, return_ms: bool = False):
    """Chain Q4 on plain arrays: ``nn`` (m, k) indices into the rows of ``Yref`` (n, 2 or 3), ``w`` (m, k) weights (finite,
    >= 0, a positive one in every row), ``init`` the (m, c) start; ``alpha0`` is the initial step itself.  Only the queries
    move.  Row i draws its negatives as query ``first_index + i``: a slice of a larger call is reproduced bit for bit."""
    nn, w = np.asarray(nn), np.asarray(w)
    if nn.ndim != 2 or nn.dtype.kind not in "iu" or not 1 <= nn.shape[1] <= 64 or nn.shape[0] < 1:
        raise ValueError("nn must be an (m, k) integer array with m >= 1 and 1 <= k <= 64")
    if w.shape != nn.shape or w.dtype.kind not in "fiu":
        raise ValueError("w must be a numeric array of nn's shape %s" % (nn.shape,))
    Yref, Y0 = np.asarray(Yref), np.asarray(init)
    if Yref.ndim != 2 or Yref.shape[0] < 1 or Yref.shape[1] not in (2, 3) or Yref.dtype.kind not in "fiu":
        raise ValueError("Yref must be a numeric (n, 2) or (n, 3) array")
    n, c = Yref.shape
    if Y0.shape != (nn.shape[0], c) or Y0.dtype.kind not in "fiu":
        raise ValueError("init must be a numeric array of shape (%d, %d)" % (nn.shape[0], c))
    if nn.min() < 0 or nn.max() >= n:
        raise ValueError("nn must index the %d rows of Yref" % n)
    nn = np.ascontiguousarray(nn, dtype=np.int32)
    w = np.ascontiguousarray(w, dtype=np.float32)
    Yref = np.ascontiguousarray(Yref, dtype=np.float32)
    Y0 = np.ascontiguousarray(Y0, dtype=np.float32)
    if not (np.isfinite(w).all() and (w >= 0).all() and (w.max(axis=1) > 0).all()):
        raise ValueError("w must be finite and >= 0 with a positive weight in every row")
    if not (np.isfinite(Yref).all() and np.isfinite(Y0).all()):
        raise ValueError("Yref and init must be finite")
    a, b = float(a), float(b)
    if not (math.isfinite(a) and math.isfinite(b)):
        raise ValueError("a and b must be finite")
    T, alpha0, neg, seed = _check_layout_args(n_epochs, alpha0, negative_sample_rate, seed)
    q0 = first_index
    if isinstance(q0, bool) or int(q0) != q0 or q0 < 0 or int(q0) + nn.shape[0] > 2 ** 31 - 1:
        raise ValueError("first_index must be an integer >= 0 with first_index + m <= 2^31 - 1")
    out = np.empty_like(Y0)
    ms = _lib.call_ms("mi_umap_transform_layout_f32", nn.shape[0], nn.shape[1], nn, w, n, c, Yref, Y0, a, b, alpha0, T, neg,
                      C.c_uint64(seed), C.c_int64(int(q0)), int(device), out)
    return (out, ms) if return_ms else out


def transform(X_new, X_ref, model, n_neighbors: int = 30, metric: str = "cosine", n_epochs=None, learning_rate: float = 1.0,
              negative_sample_rate: int = 5, seed: int = 42, first_index: int = 0, device: int = 0) -> Result:
    """Places ``X_new`` in the embedding ``model`` (a :class:`UmapResult`, or anything with ``coords``, ``a``, ``b``,
    ``n_epochs``) fitted on ``X_ref``, by umap-learn's transform rule: the ``n_neighbors`` nearest reference points of every
    query, membership weights with rho = 0, the weighted mean of their positions as the start, then ``n_epochs`` epochs
    (``None``: a third of the fit's, at least 1) at a quarter of ``learning_rate`` in which only the queries move.  Pass the
    fit's ``n_neighbors`` and ``metric``.  Firing ratios are normalised per row where umap-learn normalises per batch, so
    ``transform(Q)[a:b]`` equals ``transform(Q[a:b], first_index=a)`` bit for bit.  Returns ``coords``, ``init``, ``nn``,
    ``dist``, ``sigma``, ``weights``, ``n_epochs``, ``timing``."""
    from .mapping import QueryGraph, _check_pair
    t_all = time.perf_counter()
    Q, R, k = _check_pair(X_new, X_ref, n_neighbors, metric)
    try:
        Yref, a, b, fit_epochs = np.asarray(model.coords), float(model.a), float(model.b), model.n_epochs
    except AttributeError as exc:
        raise ValueError("model needs coords, a, b and n_epochs (a UmapResult): %s" % exc) from None
    if Yref.ndim != 2 or Yref.shape[0] != R.shape[0] or Yref.shape[1] not in (2, 3) or Yref.dtype.kind not in "fiu":
        raise ValueError("model.coords must be (%d, 2) or (%d, 3): one row per row of X_ref" % (R.shape[0], R.shape[0]))
    if not np.isfinite(Yref).all() or not (math.isfinite(a) and math.isfinite(b)):
        raise ValueError("model.coords, model.a and model.b must be finite")
    if n_epochs is None:
        if isinstance(fit_epochs, bool) or int(fit_epochs) != fit_epochs or fit_epochs < 1:
            raise ValueError("model.n_epochs must be a positive integer")
        n_epochs = max(1, int(fit_epochs) // 3)
    T, lr, neg, seed = _check_layout_args(n_epochs, learning_rate, negative_sample_rate, seed)
    if isinstance(first_index, bool) or int(first_index) != first_index or first_index < 0 \
            or int(first_index) + Q.shape[0] > 2 ** 31 - 1:
        raise ValueError("first_index must be an integer >= 0 with first_index + m <= 2^31 - 1")
    with QueryGraph(Q, R, k, metric, device) as g:
        nn, dist = g.fetch_knn()
        sigma, w = g.smooth().fetch_smooth()
        Y0 = g.init(Yref)
        timing = dict(g.timing)
    coords, ms = transform_layout(nn, w, Yref, Y0, a, b, lr / 4.0, T, neg, seed, first_index, device, return_ms=True)
    timing["layout_ms"] = ms
    total_ms = (time.perf_counter() - t_all) * 1e3
    timing["host_ms"] = total_ms - sum(timing[s] for s in ("knn_ms", "smooth_ms", "init_ms", "layout_ms"))
    timing["total_ms"] = total_ms
    return Result(coords=coords, init=Y0, nn=nn, dist=dist, sigma=sigma, weights=w, n_epochs=T, timing=timing)
