"""t-SNE on the GPU: points -> exact kNN (K = floor(3 perplexity), in passes of 64) -> perplexity calibration -> the joint
distribution P as a symmetric CSR -> a layout whose repulsion is the exact all-pairs sum.  The twin of the UMAP picture in the
reference's normalisation notebook, in R (Seurat): `R/pbmc3k/Pbmc3k_normalization_simulated_data.Rmd:236-237, 254-255,
272-273, 498`: ``RunUMAP(obj, reduction = "pca", dims = 1:10)`` then ``RunTSNE(obj, reduction = "pca", dims = 1:10)``.

Everything numeric past the argument checks runs in libmi_sa.so (csrc/tsne_kernels.hip, C ABI include/mi_tsne.h); the initial
coordinates are host fp64.  The chain is specified in DESIGN.md section 5d ("chain T"): every iteration is a gather from the
previous iteration's positions with fixed summation orders, so two calls return bit-identical coordinates.

Two deviations from Rtsne, both deliberate: the repulsion is exact (theta = 0) where Rtsne approximates it with a Barnes-Hut
tree at theta = 0.5, and the mean of the coordinates is removed once, after the last iteration of a call, not every iteration.
Agreement with R's Rtsne is not pinned (another generator for the start, Barnes-Hut there).

    emb = preprocess.embed(counts, nfeatures=2000, npcs=50)
    ts = tsne.run_tsne(emb.coords[:, :10])            # Seurat's RunTSNE(dims = 1:10) defaults
    outputs.plot_and_save_embedding(ts.coords, labels, "tsne.png")
"""
from __future__ import annotations

import ctypes as C
import math
import time

import numpy as np

from . import _lib
from .preprocess import Result
from .umap import pca_init

MAX_POINTS = 1 << 18                                         # MI_TSNE_MAX_POINTS
MAX_ITERS = 10000                                            # MI_TSNE_MAX_ITERS
MIN_PERPLEXITY, MAX_PERPLEXITY = 2.0, 85.0                   # MI_TSNE_MIN_PERPLEXITY, MI_TSNE_MAX_PERPLEXITY
CALIBRATION_STEPS = 100                                      # MI_TSNE_CALIBRATION_STEPS


class TsneResult(Result):
    """``coords`` (n x c f32), ``kl_divergence``, ``graph`` (the :func:`affinities` result), ``n_iter``, ``timing`` (kernel ms
    per stage, host ms) and ``kernel_ms`` (their sum)."""


def n_neighbors(perplexity) -> int:
    """K = floor(3 perplexity), the neighbours the calibration sees (Rtsne's rule)."""
    return int(math.floor(3.0 * float(perplexity)))


def chunks(n: int) -> int:
    """S(n), the number of pieces k_tsne_repulse cuts the j axis into: the largest power of two <= n / 64, between 1 and 16
    (a function of n alone)."""
    S = 1
    while S < 16 and 2 * S * 64 <= int(n):
        S *= 2
    return S


def lanes(nnz: int, n: int) -> int:
    """G, the lanes of k_tsne_update that own one point: the smallest of 16, 32, 64 that holds the mean row length."""
    mean = nnz / n
    return 64 if mean > 32.0 else (32 if mean > 16.0 else 16)


# ---- argument checks (all before any ctypes call) ---------------------------------------------------------------------------

def _check_points(X, perplexity):
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError("X must be (n, dim) (got shape %s)" % (X.shape,))
    if X.dtype.kind not in "fiu":
        raise ValueError("X must be numeric")
    X = np.ascontiguousarray(X, dtype=np.float32)
    n, dim = X.shape
    if not 1 <= dim <= 64:
        raise ValueError("need 1 <= dim <= 64 (got %d)" % dim)
    if isinstance(perplexity, bool):
        raise ValueError("perplexity must be a number")
    perplexity = float(perplexity)
    if not MIN_PERPLEXITY <= perplexity <= MAX_PERPLEXITY:
        raise ValueError("need %g <= perplexity <= %g (got %r)" % (MIN_PERPLEXITY, MAX_PERPLEXITY, perplexity))
    if n < 2 or n_neighbors(perplexity) > n - 1:
        raise ValueError("perplexity is too large: floor(3 * %g) = %d neighbours, n - 1 = %d"
                         % (perplexity, n_neighbors(perplexity), n - 1))
    if n > MAX_POINTS:
        raise ValueError("n = %d exceeds %d (the repulsion is n^2 per iteration)" % (n, MAX_POINTS))
    if not np.isfinite(X).all():
        raise ValueError("X must be finite")
    return X, perplexity


def _check_csr(rowptr, col, P):
    rowptr = np.asarray(rowptr)
    col, P = np.asarray(col), np.asarray(P)
    if rowptr.ndim != 1 or len(rowptr) < 2 or rowptr.dtype.kind not in "iu":
        raise ValueError("rowptr must be a 1-d integer array of n + 1 entries")
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
    if col.ndim != 1 or col.dtype.kind not in "iu" or P.ndim != 1 or P.dtype.kind not in "fiu":
        raise ValueError("col must be a 1-d integer array and P a 1-d numeric array")
    if len(col) != rowptr[-1] or len(P) != rowptr[-1]:
        raise ValueError("col and P must have rowptr[-1] = %d entries" % rowptr[-1])
    if len(col) and (col.min() < -2 ** 31 or col.max() >= 2 ** 31):
        raise ValueError("column index out of range")
    return rowptr, np.ascontiguousarray(col, dtype=np.int32), np.ascontiguousarray(P, dtype=np.float32)


def _check_coords(Y, n, what):
    Y = np.asarray(Y)
    if Y.ndim != 2 or Y.shape[0] != n or Y.dtype.kind not in "fiu":
        raise ValueError("%s must be a numeric (n, n_components) array with n = %d" % (what, n))
    return np.ascontiguousarray(Y, dtype=np.float32)


def _check_int(v, lo, hi, what):
    if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= hi:
        raise ValueError("%s must be an integer in [%d, %d] (got %r)" % (what, lo, hi, v))
    return int(v)


def _check_layout_args(n_iter, learning_rate, early_exaggeration, exaggeration_iters, momentum, momentum_switch_iter,
                       first_iter):
    T = _check_int(n_iter, 1, MAX_ITERS, "n_iter")
    t0 = _check_int(first_iter, 0, 2 ** 31 - 1 - T, "first_iter")
    ex_iters = _check_int(exaggeration_iters, 0, 2 ** 31 - 1, "exaggeration_iters")
    sw_iter = _check_int(momentum_switch_iter, 0, 2 ** 31 - 1, "momentum_switch_iter")
    eta, ex = float(learning_rate), float(early_exaggeration)
    if not (math.isfinite(eta) and eta > 0.0):
        raise ValueError("learning_rate must be finite and > 0")
    if not (math.isfinite(ex) and ex > 0.0):
        raise ValueError("early_exaggeration must be finite and > 0")
    try:
        m0, m1 = (float(v) for v in momentum)
    except (TypeError, ValueError):
        raise ValueError("momentum must be a pair (before, after momentum_switch_iter)") from None
    if not (math.isfinite(m0) and math.isfinite(m1)):
        raise ValueError("momentum must be finite")
    return T, t0, eta, ex, ex_iters, m0, m1, sw_iter


# ---- device passes -------------------------------------------------------------------------------------------------------------

class Affinities(_lib.Handle):
    """The handle of include/mi_tsne.h: T1 on construction, then :meth:`calibrate` and :meth:`symmetrize`.  A context manager;
    ``timing`` collects the device milliseconds of every pass that has run."""
    _destroy = "mi_tsne_destroy"

    def __init__(self, X, perplexity: float = 30.0, device: int = 0):
        X, perplexity = _check_points(X, perplexity)
        self.n, self.dim, self.K = X.shape[0], X.shape[1], n_neighbors(perplexity)
        self.perplexity, self.device = perplexity, int(device)
        self.timing = {}
        h = C.c_void_p()
        self.timing["knn_ms"] = _lib.call_ms("mi_tsne_knn_f32", X, self.n, self.dim, perplexity, self.device, h)
        self._h = h

    def fetch_knn(self):
        """``(nn, d2)``: n x K int32 indices of the nearest other points and n x K f32 squared distances, ascending
        (d2, index)."""
        nn = np.empty((self.n, self.K), dtype=np.int32)
        d2 = np.empty((self.n, self.K), dtype=np.float32)
        _lib.call("mi_tsne_fetch_knn", self._handle(), nn, d2)
        return nn, d2

    def calibrate(self):
        self.timing["calibrate_ms"] = _lib.call_ms("mi_tsne_calibrate", self._handle())
        return self

    def fetch_beta(self, conditional: bool = False):
        """``beta`` (n fp64); with ``conditional`` also the n x K conditional rows p_j|i, rounded to f32."""
        beta = np.empty(self.n)
        cond = np.empty((self.n, self.K), dtype=np.float32) if conditional else None
        _lib.call("mi_tsne_fetch_calibration", self._handle(), beta, cond)
        return (beta, cond) if conditional else beta

    def symmetrize(self):
        self.timing["symmetrize_ms"] = _lib.call_ms("mi_tsne_symmetrize", self._handle())
        return self

    def info(self) -> dict:
        nnz, deg = C.c_int64(0), C.c_int(0)
        _lib.call("mi_tsne_info", self._handle(), None, None, nnz, deg)
        return {"nnz": int(nnz.value), "max_degree": int(deg.value)}

    def fetch_graph(self):
        """``(rowptr, col, P)``: the symmetric CSR (int64, int32, f32), rows ascending by column."""
        rowptr = np.empty(self.n + 1, dtype=np.int64)
        _lib.call("mi_tsne_fetch_graph", self._handle(), rowptr, None, None)
        col = np.empty(int(rowptr[-1]), dtype=np.int32)
        P = np.empty(int(rowptr[-1]), dtype=np.float32)
        _lib.call("mi_tsne_fetch_graph", self._handle(), None, col, P)
        return rowptr, col, P


def affinities(X, perplexity: float = 30.0, device: int = 0) -> Result:
    """Chain T1 - T3: ``nn``, ``d2``, ``beta``, ``cond``, ``rowptr``, ``col``, ``P``, ``max_degree``, ``timing``."""
    with Affinities(X, perplexity, device) as g:
        nn, d2 = g.fetch_knn()
        beta, cond = g.calibrate().fetch_beta(conditional=True)
        rowptr, col, P = g.symmetrize().fetch_graph()
        return Result(nn=nn, d2=d2, beta=beta, cond=cond, rowptr=rowptr, col=col, P=P, max_degree=g.info()["max_degree"],
                      timing=dict(g.timing))


def layout(rowptr, col, P, init, n_iter: int = 1000, learning_rate: float = 200.0, early_exaggeration: float = 12.0,
           exaggeration_iters: int = 250, momentum=(0.5, 0.8), momentum_switch_iter: int = 250, state=None,
           first_iter: int = 0, return_state: bool = False, center: bool = True, device: int = 0, return_ms: bool = False):
    """Chain T4 on any symmetric CSR with positive finite weights: ``init`` is the (n, 2) or (n, 3) start; iterations
    ``first_iter .. first_iter + n_iter - 1`` of bhtsne's update with the exact repulsion.  ``state``: ``(U, gains)`` of an
    earlier call (None: velocity 0, gains 1).  ``center``: subtract the column means once, after the last iteration.  A run of
    T iterations equals a run of T1 with ``center=False`` followed by one of T - T1 with ``first_iter=T1`` and the first
    run's coordinates and state, bit for bit.  Returns the coordinates; with ``return_state`` ``(coords, (U, gains), Z)``, Z
    the last iteration's normaliser; with ``return_ms`` the kernels' ms is appended."""
    rowptr, col, P = _check_csr(rowptr, col, P)
    n = len(rowptr) - 1
    Y0 = _check_coords(init, n, "init")
    U = G = None
    if state is not None:
        try:
            U, G = state
        except (TypeError, ValueError):
            raise ValueError("state must be (U, gains)") from None
        U, G = _check_coords(U, n, "state[0]"), _check_coords(G, n, "state[1]")
        if U.shape != Y0.shape or G.shape != Y0.shape:
            raise ValueError("state arrays must have init's shape %s" % (Y0.shape,))
    T, t0, eta, ex, ex_iters, m0, m1, sw_iter = _check_layout_args(n_iter, learning_rate, early_exaggeration,
                                                                   exaggeration_iters, momentum, momentum_switch_iter,
                                                                   first_iter)
    out = np.empty_like(Y0)
    U_out, G_out, Z = (np.empty_like(Y0), np.empty_like(Y0), C.c_double(0.0)) if return_state else (None, None, None)
    ms = _lib.call_ms("mi_tsne_layout_f32", n, Y0.shape[1], rowptr, col, P, Y0, U, G, eta, ex, ex_iters, m0, m1, sw_iter, T, t0,
                      1 if center else 0, int(device), out, U_out, G_out, Z)
    res = (out, (U_out, G_out), float(Z.value)) if return_state else out
    if return_ms:
        return res + (ms,) if return_state else (out, ms)
    return res


def kl_divergence(rowptr, col, P, Y, device: int = 0, return_ms: bool = False):
    """KL(P || Q) at ``Y``: sum over the stored entries of ``P log(P Z / q)`` with the exact Z, fp64 sums in a fixed order
    (bit-identical between calls); Rtsne's final ``itercosts``, summed."""
    rowptr, col, P = _check_csr(rowptr, col, P)
    Y = _check_coords(Y, len(rowptr) - 1, "Y")
    kl = C.c_double(0.0)
    ms = _lib.call_ms("mi_tsne_kl_f32", len(rowptr) - 1, Y.shape[1], rowptr, col, P, Y, int(device), kl)
    return (float(kl.value), ms) if return_ms else float(kl.value)


def random_init(n: int, n_components: int = 2, seed: int = 1) -> np.ndarray:
    """``1e-4 * np.random.default_rng(seed).standard_normal((n, c))`` as f32 (bhtsne's scale, numpy's generator)."""
    return (1e-4 * np.random.default_rng(seed).standard_normal((int(n), int(n_components)))).astype(np.float32)


def scaled_pca_init(X, n_components: int = 2) -> np.ndarray:
    """:func:`umap.pca_init` rescaled by one factor so that its first column has standard deviation 1e-4 (population
    formula, fp64); a constant first column leaves zeros."""
    Y = pca_init(X, n_components).astype(np.float64)
    sd = float(Y[:, 0].std())
    return np.ascontiguousarray(Y * (1e-4 / sd) if sd > 0.0 else Y * 0.0, dtype=np.float32)


def run_tsne(X, perplexity: float = 30.0, n_components: int = 2, n_iter: int = 1000, learning_rate: float = 200.0,
             early_exaggeration: float = 12.0, exaggeration_iters: int = 250, momentum=(0.5, 0.8),
             momentum_switch_iter: int = 250, init="random", seed: int = 1, device: int = 0) -> TsneResult:
    """Seurat's ``RunTSNE`` (Rtsne's defaults: perplexity 30, 1000 iterations, eta 200, exaggeration 12 for 250 iterations,
    momentum 0.5 then 0.8) on ``X`` = the PCA coordinates (``emb.coords[:, :10]`` for ``dims = 1:10``), with the exact
    repulsion.  ``init``: ``"random"`` (:func:`random_init` of ``seed``), ``"pca"`` (:func:`scaled_pca_init`) or an
    (n, n_components) array.  Two calls with the same arguments return bit-identical coordinates."""
    t_all = time.perf_counter()
    X, perplexity = _check_points(X, perplexity)
    n = X.shape[0]
    if isinstance(n_components, bool) or n_components not in (2, 3):
        raise ValueError("n_components must be 2 or 3 (got %r)" % (n_components,))
    c = int(n_components)
    _check_layout_args(n_iter, learning_rate, early_exaggeration, exaggeration_iters, momentum, momentum_switch_iter, 0)
    if isinstance(init, str):
        if init == "random":
            if isinstance(seed, bool) or int(seed) != seed or seed < 0:
                raise ValueError("seed must be an integer >= 0")
            Y0 = random_init(n, c, int(seed))
        elif init == "pca":
            Y0 = scaled_pca_init(X, c)
        else:
            raise ValueError("init must be 'random', 'pca' or an (n, n_components) array")
    else:
        Y0 = _check_coords(init, n, "init")
        if Y0.shape != (n, c) or not np.isfinite(Y0).all():
            raise ValueError("init must be a finite array of shape (%d, %d)" % (n, c))
    g = affinities(X, perplexity, device)
    coords, ms = layout(g.rowptr, g.col, g.P, Y0, n_iter, learning_rate, early_exaggeration, exaggeration_iters, momentum,
                        momentum_switch_iter, device=device, return_ms=True)
    kl, kl_ms = kl_divergence(g.rowptr, g.col, g.P, coords, device, return_ms=True)
    timing = dict(g.timing)
    timing["layout_ms"] = ms
    timing["iter_ms"] = ms / int(n_iter)
    timing["kl_ms"] = kl_ms
    kernel_ms = sum(timing[s] for s in ("knn_ms", "calibrate_ms", "symmetrize_ms", "layout_ms", "kl_ms"))
    total_ms = (time.perf_counter() - t_all) * 1e3
    timing["host_ms"] = total_ms - kernel_ms
    timing["total_ms"] = total_ms
    return TsneResult(coords=coords, kl_divergence=kl, graph=g, n_iter=int(n_iter), timing=timing, kernel_ms=kernel_ms)
