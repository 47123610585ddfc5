"""Preprocessing on the GPU: counts -> log-normalised matrix -> variable genes -> scaled matrix -> PCA coordinates, the
input of :func:`snn.build_snn`; the normalised matrix is the one :func:`metrics.find_all_markers` takes.

This is the first chunk of every data-preparation notebook of the reference, in R
(`R/pbmc3k/Pbmc3k_normalization_simulated_data.Rmd:81-82,184-185,488-492`: Seurat's ``NormalizeData(LogNormalize, 1e4)`` ->
``FindVariableFeatures("vst")`` -> ``ScaleData`` -> ``RunPCA``; `Pbmc3k_prepare_data_for_QA_clustering.Rmd:51-52`,
`Kidney_data.Rmd:47-48`).  The passes over the cells x genes matrix and the Gram and projection products run in libmi_sa.so
(csrc/prep_kernels.hip, C ABI include/mi_prep.h); only the loess curve of ``vst`` and the h x h eigen-solve are host fp64.

Sparse counts: every entry point takes a ``scipy.sparse`` matrix or array as well; the handle then keeps the counts as CSR
plus its transpose on the device, never an n x g buffer (``n * g`` is not limited), and every result equals, bit for bit,
that of the dense handle on the densified matrix.  :func:`read_10x_mtx` reads a 10x directory into such a matrix.

Cell QC and ``vars.to.regress`` (the three lines every notebook starts with: ``PercentageFeatureSet(pattern = "^MT-")``,
``subset(nFeature_RNA > 200 & nFeature_RNA < 2500 & percent.mt < 5)``, ``ScaleData(vars.to.regress = "percent.mt")``;
`Pbmc3k_prepare_data_for_QA_clustering.Rmd:40-51`, `Kidney_data.Rmd:40-47`): :func:`cell_qc` and :func:`qc_filter` give the
per-cell columns and the mask, and ``vars_to_regress`` of :func:`scale_data`, :func:`pca` and :func:`embed` scales the
residuals of the linear model ``y ~ 1 + covariates`` per gene (device; the QR of the design is host fp64).

``SCTransform`` (the normalisation every data-preparation notebook but one uses: ``SCTransform(obj, method = "glmGamPoi",
vars.to.regress = "percent.mt")`` then ``RunPCA``; `Pbmc3k_prepare_data_for_QA_clustering.Rmd:51-52`,
`Kidney_data.Rmd:47-48`): :func:`sctransform` -- a per-gene negative-binomial regression on sequencing depth (device),
its regularisation over the genes (host fp64), Pearson residuals and their variance as the variable-gene criterion (device),
into the same Gram / eigen / project path.  The chain is this package's specification, modelled on ``sctransform::vst``;
agreement with R is UNPINNED.

``sctransform(..., return_corrected=True)`` also returns SCTransform's corrected counts and its ``data`` slot (the matrix
the reference's benchmarks measure on) as a second device handle (:meth:`ExpressionMatrix.sct_correct`).

Out of scope: ``vst.flavor = "v2"``, ``batch_var``, a corrected matrix restricted to Seurat's gene subset, latent variables
other than ``log_umi``, glmGamPoi's Cox-Reid adjustment; more than ``MAX_FEATURES`` = 4096 features or ``MAX_COVARIATES`` = 8
covariates, sparse input to the ``--counts`` option of ``run``.

    qc = preprocess.cell_qc(counts, gene_names)
    keep = preprocess.qc_filter(qc)
    emb = preprocess.embed(counts[keep], nfeatures=2000, npcs=50, vars_to_regress=qc.percent[keep])
    g = snn.build_snn(emb.coords[:, :15], k=5, ord=15)
"""
from __future__ import annotations

import ctypes as C
import math
import os
import re
import sys
import time
from typing import Optional

import numpy as np

from . import _lib

MAX_FEATURES = 4096        # MI_PREP_MAX_FEATURES (include/mi_prep.h)
MAX_PCS = 128              # MI_PREP_MAX_PCS
GRAM_CHUNK = 512           # MI_PREP_GRAM_CHUNK
GRAM_WORKSPACE = 256 << 20  # MI_PREP_GRAM_WORKSPACE: bytes of f32 chunk tiles (128 x 128) one pass of gram() keeps in flight
MAX_COVARIATES = 8         # MI_PREP_MAX_DESIGN_COLS - 1 (the intercept)

MAX_NNZ = 2 ** 31 - 1      # MI_PREP_MAX_NNZ

def is_sparse(X) -> bool:
    """Is ``X`` a ``scipy.sparse`` matrix or array (scipy is imported only if the caller has done so)"""
    sp = sys.modules.get("scipy.sparse")
    return sp is not None and sp.issparse(X)


def canonical_csr(X):
    """``(indptr int64, indices int32, data float32, (n, g))`` of a ``scipy.sparse`` matrix or array of any format, as
    ``mi_prep_create_csr_f32`` takes it: CSR, duplicates summed, the columns of every row ascending.  Stored zeros are kept.
    ``X`` is not modified.  Host only (no library load).  ``ValueError`` for ``g >= 2^31``."""
    if not is_sparse(X):
        raise ValueError("X must be a scipy.sparse matrix or array")
    if X.ndim != 2:
        raise ValueError("X must be (cells, genes) (got shape %s)" % (X.shape,))
    n, g = (int(s) for s in X.shape)
    if g >= 2 ** 31:
        raise ValueError("%d genes: column indices must fit 32 bits" % g)
    A = X.tocsr()
    if not A.has_canonical_format:
        A = A.copy() if A is X else A
        A.sum_duplicates()                                       # (sorts the indices as well)
    return (np.ascontiguousarray(A.indptr, dtype=np.int64), np.ascontiguousarray(A.indices, dtype=np.int32),
            np.ascontiguousarray(A.data, dtype=np.float32), (n, g))


class ExpressionMatrix(_lib.Handle):
    """A cells x genes count matrix resident on the GPU (uploaded once), with one method per pass of include/mi_prep.h.
    ``X`` is a dense array or a ``scipy.sparse`` matrix / array (``sparse`` tells which; ``nnz``: its stored entries, ``n * g``
    for a dense one).  A context manager; ``timing`` collects the device milliseconds of every pass that has run."""
    _destroy = "mi_prep_destroy"

    def __init__(self, X, device: int = 0):
        self.sparse = is_sparse(X)
        if self.sparse:
            self._indptr, self._indices, data, shape = canonical_csr(X)
        else:
            X = np.ascontiguousarray(X, dtype=np.float32)
            if X.ndim != 2:
                raise ValueError("X must be (cells, genes) (got shape %s)" % (X.shape,))
            shape = X.shape
        self.n, self.g = (int(s) for s in shape)
        self.nnz = len(data) if self.sparse else self.n * self.g
        self.device = int(device)
        self.h = 0
        self.normalized = False                                  # has normalize() run
        self.timing = {}
        self._stats = {}
        self.coef_q = self.resid_mean = self.resid_var = self.flat = self.regression = None     # of select_regressed
        self._lib = _lib.load()
        h = C.c_void_p()
        if self.sparse:
            t0 = time.perf_counter()
            _lib.call("mi_prep_create_csr_f32", self._indptr, self._indices, data, self.n, self.g, self.device, h)
            self.timing["create_s"] = time.perf_counter() - t0   # the checks, the transpose (host) and the upload
        else:
            _lib.call("mi_prep_create_f32", X, self.n, self.g, self.device, h)
        self._h = h

    @classmethod
    def _adopt(cls, lib, h, device: int) -> "ExpressionMatrix":
        """An open handle around a ``mi_prep_matrix *`` the library has created (``mi_prep_sct_correct``): shape and kind
        come from ``mi_prep_info``, a sparse handle's structure from ``mi_prep_fetch_csr``.  Closes it if that fails."""
        m = cls.__new__(cls)
        m._lib, m._h, m.device = lib, h, int(device)
        m.h, m.normalized, m.timing, m._stats = 0, True, {}, {}
        m.coef_q = m.resid_mean = m.resid_var = m.flat = m.regression = None
        try:
            n, g, sparse, nnz = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
            _lib.call("mi_prep_info", h, n, g, nnz, sparse, None)
            m.n, m.g, m.nnz, m.sparse = int(n.value), int(g.value), int(nnz.value), bool(sparse.value)
            if m.sparse:
                m._indptr, m._indices = np.empty(m.n + 1, dtype=np.int64), np.empty(m.nnz, dtype=np.int32)
                _lib.call("mi_prep_fetch_csr", h, m._indptr, m._indices, None)
        except Exception:
            m.close()
            raise
        return m

    def device_bytes(self) -> int:
        """Bytes the handle holds resident on the device now."""
        out = C.c_int64(0)
        _lib.call("mi_prep_info", self._handle(), None, None, None, None, out)
        return int(out.value)

    def normalize(self, scale_factor: float = 1e4):
        """Seurat's ``LogNormalize``: ``log1p(x * scale_factor / total of the cell)``, kept on the device.  A cell without
        counts keeps zeros (Seurat returns NaN there)."""
        ms = _lib.call_ms("mi_prep_normalize", self._handle(), float(scale_factor))
        self._stats.pop(1, None)
        self.normalized = True
        self.timing["normalize_ms"] = ms
        return self

    def fetch_normalized(self):
        """The normalised matrix: an ndarray (n x g, fp32), or for a sparse handle a ``csr_matrix`` with the uploaded
        structure (stored zeros included) and fp32 data."""
        if self.sparse:
            from scipy.sparse import csr_matrix
            data = np.empty(self.nnz, dtype=np.float32)
            _lib.call("mi_prep_fetch_normalized_csr", self._handle(), data)
            return csr_matrix((data, self._indices, self._indptr), shape=(self.n, self.g))
        out = np.empty((self.n, self.g), dtype=np.float32)
        _lib.call("mi_prep_fetch_normalized", self._handle(), out)
        return out

    def fetch_counts(self):
        """The counts the handle holds: an ndarray (n x g, fp32), or for a sparse handle a ``csr_matrix`` with the handle's
        structure and fp32 data."""
        if self.sparse:
            from scipy.sparse import csr_matrix
            data = np.empty(self.nnz, dtype=np.float32)
            _lib.call("mi_prep_fetch_csr", self._handle(), None, None, data)
            return csr_matrix((data, self._indices, self._indptr), shape=(self.n, self.g))
        out = np.empty((self.n, self.g), dtype=np.float32)
        _lib.call("mi_prep_fetch_counts", self._handle(), out)
        return out

    def gene_stats(self, which: str = "counts"):
        """``(mean, variance, nnz)`` per gene of the ``"counts"`` or the ``"normalized"`` matrix: fp64 mean, sample
        variance (ddof 1) about it, cells with a non-zero value."""
        if which not in ("counts", "normalized"):
            raise ValueError("which must be 'counts' or 'normalized'")
        w = int(which == "normalized")
        if w not in self._stats:
            mean, var = np.empty(self.g), np.empty(self.g)
            nnz = np.empty(self.g, dtype=np.int32)
            self.timing["gene_stats_%s_ms" % which] = _lib.call_ms("mi_prep_gene_stats", self._handle(), w, mean, var, nnz)
            self._stats[w] = (mean, var, nnz)
        return self._stats[w]

    def clipped_variance(self, mean, sd, clip: float) -> np.ndarray:
        """``sum_i min((x_ij - mean_j) / sd_j, clip)^2 / (n - 1)`` over the counts, 0 where ``sd_j == 0`` (the second pass
        of ``vst``)."""
        mean = np.ascontiguousarray(mean, dtype=np.float64)
        sd = np.ascontiguousarray(sd, dtype=np.float64)
        if mean.shape != (self.g,) or sd.shape != (self.g,):
            raise ValueError("mean and sd must have one entry per gene (%d)" % self.g)
        out = np.empty(self.g)
        self.timing["clipped_variance_ms"] = _lib.call_ms("mi_prep_clipped_variance", self._handle(), mean, sd, float(clip),
                                                          out)
        return out

    def select(self, genes, mu, sigma, clip: float = 10.0):
        """Materialises ``Z[:, c] = fminf((y[:, genes[c]] - f32(mu[c])) * f32(1 / sigma[c]), f32(clip))`` (0 where
        ``sigma[c] == 0``) on the device; :meth:`fetch_scaled`, :meth:`gram` and :meth:`project` read it."""
        genes = self._index_array(genes, "genes", "gene index out of range")
        mu = np.ascontiguousarray(mu, dtype=np.float64)
        sigma = np.ascontiguousarray(sigma, dtype=np.float64)
        if mu.shape != genes.shape or sigma.shape != genes.shape:
            raise ValueError("mu and sigma must have one entry per chosen gene")
        self.h = 0
        ms = _lib.call_ms("mi_prep_select", self._handle(), genes, len(genes), mu, sigma, float(clip))
        self.h = len(genes)
        self.timing["select_ms"] = ms
        return self

    def cell_qc(self, gene_mask=None):
        """``(n_count, n_feature, subset_count)`` per cell of the counts: the fp64 total (the one :meth:`normalize` divides
        by), the genes with a non-zero count, and the total over the genes of ``gene_mask`` (g booleans; ``None`` without
        a mask)."""
        mask = None
        if gene_mask is not None:
            mask = np.asarray(gene_mask)
            if mask.dtype != np.bool_ or mask.shape != (self.g,):
                raise ValueError("gene_mask must be a boolean array with one entry per gene (%d)" % self.g)
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
        n_count, n_feature = np.empty(self.n), np.empty(self.n, dtype=np.int32)
        subset = None if mask is None else np.empty(self.n)
        self.timing["qc_ms"] = _lib.call_ms("mi_prep_cell_qc", self._handle(), mask, n_count, n_feature, subset)
        return n_count, n_feature, subset

    def rank_sum_pass(self, L, K: int, which: str = "normalized", plain: bool = False, force_global: bool = False,
                      gather: Optional[str] = None) -> dict:
        """The device pass of :func:`metrics.rank_sum_pass` on the resident ``"counts"`` or ``"normalized"`` matrix, with no
        upload and, on a sparse handle, no n x g buffer: the same dict (``rank2``, ``npos``, ``sum``, ``tie``,
        ``kernel_ms``), bit for bit that of the dense entry point on the densified matrix.  ``gather`` (sparse handle only;
        changes no result): ``"permute"`` copies the values into gene-major order first, ``"inplace"`` reads them through
        the position map, ``None`` takes the library's default.  The handle is not modified."""
        if which not in ("counts", "normalized"):
            raise ValueError("which must be 'counts' or 'normalized'")
        if gather not in (None, "permute", "inplace"):
            raise ValueError("gather must be None, 'permute' or 'inplace'")
        L = np.asarray(L)
        if L.ndim == 1:
            L = L[None, :]
        if L.ndim != 2 or L.shape[1] != self.n:
            raise ValueError("L must be (n,) or (B, n) for the %d cells of the handle (got %s)" % (self.n, L.shape))
        if L.dtype.kind not in "iub" or (L.size and (L.min() < 0 or L.max() > 65535)):
            raise ValueError("labels must be integers in [0, K)")
        L = np.ascontiguousarray(L, dtype=np.uint16)
        B, K = L.shape[0], int(K)
        h = self._handle()
        shape = (B, self.g, max(K, 0))
        rank2, npos = np.empty(shape, dtype=np.int64), np.empty(shape, dtype=np.int32)
        sums, tie = np.empty(shape, dtype=np.float64), np.empty(self.g, dtype=np.int64)
        flags = (1 if plain else 0) | (2 if force_global else 0) | {None: 0, "inplace": 4, "permute": 8}[gather]
        ms = _lib.call_ms("mi_prep_rank_sum_markers", h, int(which == "normalized"), L, B, K, flags, rank2, npos, sums, tie)
        self.timing["markers_ms"] = ms
        return {"rank2": rank2, "npos": npos, "sum": sums, "tie": tie, "kernel_ms": ms}

    def annotate(self, gene_names, ref, **kw) -> dict:
        """:func:`annotate.single_r` on this handle, read where it is (``which="normalized"`` by default; ``clusters=``
        annotates cluster means)."""
        from . import annotate
        return annotate.single_r(self, gene_names, ref, **kw)

    def select_regressed(self, genes, Q, clip: float = 10.0):
        """:meth:`select` on the residuals of a linear model: with ``y`` the chosen column of the normalised matrix and
        ``Q`` (n, q) an orthonormal basis of the design (:func:`design_basis`), ``r = y - Q (Q^T y)`` and
        ``Z[:, c] = f32(min((r - mean(r)) / sd(r), clip))`` in fp64 with one rounding, 0 for a flat column
        (``sum (r - mean)^2 <= 1e-16 sum y^2``: an all-zero gene, a constant gene, a gene in the span of the design).
        Stores ``coef_q`` (q, h: ``Q^T y``), ``resid_mean``, ``resid_var`` and ``flat`` (h each) on the handle."""
        genes = self._index_array(genes, "genes", "gene index out of range")
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        if Q.ndim != 2 or Q.shape[0] != self.n:
            raise ValueError("Q must be (n, q) with n = %d (got shape %s)" % (self.n, Q.shape))
        h, q = len(genes), Q.shape[1]
        coef, mean, var = np.empty((max(q, 1), max(h, 1))), np.empty(max(h, 1)), np.empty(max(h, 1))
        flat = np.empty(max(h, 1), dtype=np.uint8)
        self.h = 0
        ms = _lib.call_ms("mi_prep_select_regressed", self._handle(), genes, h, Q, q, float(clip), coef, mean, var, flat)
        self.h = h
        self.coef_q, self.resid_mean, self.resid_var, self.flat = coef, mean, var, flat.astype(bool)
        self.timing["regress_ms"] = ms
        return self

    def gene_log1p_sum(self) -> np.ndarray:
        """``sum_i log1p(x_ij)`` per gene of the counts, fp64 (``expm1`` of it over n is sctransform's geometric mean)."""
        out = np.empty(self.g)
        self.timing["gene_log1p_ms"] = _lib.call_ms("mi_prep_gene_log1p_sum", self._handle(), out)
        return out

    @staticmethod
    def _index_array(idx, what, out_of_range=None):
        idx = np.asarray(idx)
        if idx.ndim != 1 or idx.dtype.kind not in "iu":
            raise ValueError("%s must be a 1-d integer array" % what)
        if len(idx) and (idx.min() < -2 ** 31 or idx.max() >= 2 ** 31):
            raise ValueError(out_of_range or "%s: index out of range" % what)
        return np.ascontiguousarray(idx, dtype=np.int32)

    def nb_fit(self, cells, genes, log_umi) -> "Result":
        """The negative-binomial regression of SCTransform's step 1 on the device (``mi_prep_nb_fit``; the algorithm is in
        include/mi_prep.h): per gene of ``genes``, over ``cells``, ``y ~ NB(mu, alpha)`` with ``log mu = b0 + b1 log_umi``.
        ``log_umi``: one entry per entry of ``cells``.  Returns ``b0``, ``b1``, ``alpha``, ``se_b0c``, ``se_b1``,
        ``se_alpha``, ``iterations``, ``converged``, ``poisson`` (one entry per gene) and ``log_umi_mean``."""
        cells, genes = self._index_array(cells, "cells"), self._index_array(genes, "genes")
        log_umi = np.ascontiguousarray(log_umi, dtype=np.float64)
        if log_umi.shape != cells.shape:
            raise ValueError("log_umi must have one entry per fit cell (%d)" % len(cells))
        if not np.isfinite(log_umi).all():
            raise ValueError("log_umi must be finite: a cell without counts cannot be fitted (run qc_filter first)")
        k = max(len(genes), 1)
        f = [np.empty(k) for _ in range(6)]
        it, conv, pois = np.empty(k, dtype=np.int32), np.empty(k, dtype=np.uint8), np.empty(k, dtype=np.uint8)
        self.timing["nb_fit_ms"] = _lib.call_ms("mi_prep_nb_fit", self._handle(), cells, len(cells), genes, len(genes), log_umi,
                                                *f, it, conv, pois)
        total = 0.0
        for v in log_umi.tolist():                               # (the entry's mean: the sum in this order)
            total += v
        return Result(b0=f[0], b1=f[1], alpha=f[2], se_b0c=f[3], se_b1=f[4], se_alpha=f[5], iterations=it,
                      converged=conv.astype(bool), poisson=pois.astype(bool), log_umi_mean=total / len(log_umi))

    def _nb_parameters(self, genes, b0, b1, alpha, log_umi):
        genes = self._index_array(genes, "genes")
        par = [np.ascontiguousarray(a, dtype=np.float64) for a in (b0, b1, alpha)]
        if any(a.shape != genes.shape for a in par):
            raise ValueError("b0, b1 and alpha must have one entry per chosen gene")
        log_umi = np.ascontiguousarray(log_umi, dtype=np.float64)
        if log_umi.shape != (self.n,):
            raise ValueError("log_umi must have one entry per cell (%d)" % self.n)
        if not np.isfinite(log_umi).all():
            raise ValueError("log_umi must be finite: a cell without counts has no residual (run qc_filter first)")
        return genes, par, log_umi

    def sct_residual_moments(self, genes, b0, b1, alpha, log_umi, clip: Optional[float] = None):
        """``(mean, variance)`` (ddof 1) per chosen gene of the Pearson residual ``(x - mu) / sqrt(mu + alpha mu^2)``,
        ``mu = exp(b0 + b1 log_umi)``, clipped to ``+-clip`` (default ``sqrt(n)``), over all cells."""
        genes, par, log_umi = self._nb_parameters(genes, b0, b1, alpha, log_umi)
        clip = math.sqrt(self.n) if clip is None else float(clip)
        k = max(len(genes), 1)
        mean, var = np.empty(k), np.empty(k)
        self.timing["sct_moments_ms"] = _lib.call_ms("mi_prep_sct_residual_moments", self._handle(), genes, len(genes), par[0],
                                                     par[1], par[2], log_umi, clip, mean, var)
        return mean, var

    def sct_correct(self, genes, b0, b1, alpha, log_umi, log_umi_ref: float) -> "ExpressionMatrix":
        """SCTransform's corrected counts and ``data`` slot as a second open handle of this kind and shape, made on the
        device (``mi_prep_sct_correct``, where the formula stands): per listed gene the unclipped Pearson residual of each
        count under ``mu = exp(b0 + b1 log_umi)`` is carried to the depth ``log_umi_ref`` and rounded,
        ``c = max(rint(mu_ref + r sd_ref), 0)``; the result's counts are ``c``, its normalised matrix is ``log1p(c)``
        (``normalized`` is set: :func:`metrics.find_all_markers` ranks it where it lies).  A gene that is not listed gives
        all zeros -- the g columns stay, so gene names stay aligned.  A corrected zero need not stay zero: a sparse result
        has its own structure.  This handle is not modified and may be closed first; the caller closes the result.
        Records ``timing["sct_correct_ms"]`` here."""
        genes, par, log_umi = self._nb_parameters(genes, b0, b1, alpha, log_umi)
        out = C.c_void_p()
        self.timing["sct_correct_ms"] = _lib.call_ms("mi_prep_sct_correct", self._handle(), genes, len(genes), par[0], par[1],
                                                     par[2], log_umi, float(log_umi_ref), out)
        return ExpressionMatrix._adopt(self._lib, out, self.device)

    def select_pearson(self, genes, b0, b1, alpha, log_umi, Q=None, clip: Optional[float] = None, center: bool = True):
        """SCTransform's ``scale.data`` as ``Z``: the Pearson residuals of the chosen genes clipped to ``+-clip`` (default
        ``sqrt(n / 30)``) and rounded to float32, then projected off ``Q`` (n, q) -- the basis of ``[1]`` when ``None``
        (centring), of ``[1, covariates]`` (:func:`design_basis`) for ``vars.to.regress`` -- at unit scale.  Stores
        ``coef_q``, ``resid_mean``, ``resid_var`` and ``flat`` like :meth:`select_regressed`; :meth:`fetch_scaled`,
        :meth:`gram` and :meth:`project` follow.  ``center=False`` (without ``Q``) keeps the clipped residuals as they are."""
        genes, par, log_umi = self._nb_parameters(genes, b0, b1, alpha, log_umi)
        clip = math.sqrt(self.n / 30.0) if clip is None else float(clip)
        if not center:
            if Q is not None:
                raise ValueError("center=False takes no Q")
            self.h = 0
            ms = _lib.call_ms("mi_prep_sct_select", self._handle(), genes, len(genes), par[0], par[1], par[2], log_umi, clip,
                              None, 0, None, None, None, None)
            self.h = len(genes)
            self.coef_q = self.resid_mean = self.resid_var = self.flat = None
            self.timing["sct_select_ms"] = ms
            return self
        Q = np.full((self.n, 1), 1.0 / math.sqrt(self.n)) if Q is None else np.ascontiguousarray(Q, dtype=np.float64)
        if Q.ndim != 2 or Q.shape[0] != self.n:
            raise ValueError("Q must be (n, q) with n = %d (got shape %s)" % (self.n, Q.shape))
        h, q = len(genes), Q.shape[1]
        coef, mean, var = np.empty((max(q, 1), max(h, 1))), np.empty(max(h, 1)), np.empty(max(h, 1))
        flat = np.empty(max(h, 1), dtype=np.uint8)
        self.h = 0
        ms = _lib.call_ms("mi_prep_sct_select", self._handle(), genes, h, par[0], par[1], par[2], log_umi, clip, Q, q, coef,
                          mean, var, flat)
        self.h = h
        self.coef_q, self.resid_mean, self.resid_var, self.flat = coef, mean, var, flat.astype(bool)
        self.timing["sct_select_ms"] = ms
        return self

    def fetch_scaled(self) -> np.ndarray:
        out = np.empty((self.n, max(self.h, 1)), dtype=np.float32)
        _lib.call("mi_prep_fetch_scaled", self._handle(), out)
        return out

    def gram(self) -> np.ndarray:
        """``Z^T Z`` (h x h, fp64; not divided by n - 1): exactly symmetric and identical between runs."""
        out = np.empty((max(self.h, 1),) * 2)
        self.timing["gram_ms"] = _lib.call_ms("mi_prep_gram", self._handle(), out)
        return out

    def project(self, V) -> np.ndarray:
        """``Z @ V`` for ``V`` (h, p), p <= ``MAX_PCS``, accumulated in fp32."""
        V = np.ascontiguousarray(V, dtype=np.float32)
        if V.ndim != 2 or (self.h and V.shape[0] != self.h):
            raise ValueError("V must be (h, p) with h = %d (got shape %s)" % (self.h, V.shape))
        out = np.empty((self.n, V.shape[1]), dtype=np.float32)
        self.timing["project_ms"] = _lib.call_ms("mi_prep_project", self._handle(), V, V.shape[1], out)
        return out


class Result(dict):
    """A dict whose keys are also attributes (``emb.coords``)."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


def log_normalize(X, scale_factor: float = 1e4, device: int = 0):
    """The log-normalised fp32 matrix (cells x genes) :func:`metrics.find_all_markers` takes, dense or sparse: sparse in,
    sparse (``csr_matrix``) out.  To skip the download and the second upload, keep the handle instead:
    ``find_all_markers(ExpressionMatrix(X).normalize(), labels)`` ranks the resident matrix."""
    with ExpressionMatrix(X, device=device) as m:
        return m.normalize(scale_factor).fetch_normalized()


def loess_fit(x, y, span: float = 0.3, degree: int = 2) -> np.ndarray:
    """Local polynomial regression evaluated directly at every point, in fp64: for each ``x[i]`` the ``q = ceil(span * m)``
    nearest points (ties in distance: the lower sorted position), tricube weights ``(1 - (|dx| / d)^3)^3`` with ``d`` the
    largest of their distances, a weighted least-squares polynomial of ``degree`` in ``dx``, and its value at ``dx = 0``.
    ``span >= 1`` uses all points.  A window whose points all share ``x[i]`` gives their mean.

    R's ``loess`` (which Seurat's ``vst`` calls) evaluates the same local fits only at the vertices of a k-d tree and
    interpolates between them; R is not available to compare against, so agreement with Seurat's curve is UNPINNED."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if x.ndim != 1 or x.shape != y.shape:
        raise ValueError("x and y must be 1-d arrays of one length")
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        raise ValueError("x and y must be finite")
    if degree not in (0, 1, 2):
        raise ValueError("degree must be 0, 1 or 2")
    if not span > 0:
        raise ValueError("span must be > 0")
    m = len(x)
    q = min(m, int(math.ceil(span * m)))
    if q < degree + 1:
        raise ValueError("span * m = %d points cannot carry a polynomial of degree %d" % (q, degree))
    order = np.argsort(x, kind="stable")
    xs, ys = x[order], y[order]
    fit = np.empty(m)
    lo = 0
    for i in range(m):
        while lo + q < m and xs[lo + q] - xs[i] < xs[i] - xs[lo]:
            lo += 1
        dx = xs[lo:lo + q] - xs[i]
        d = max(-dx[0], dx[-1])
        if d == 0.0:
            fit[i] = ys[lo:lo + q].mean()
            continue
        u = dx / d
        sw = np.sqrt((1.0 - np.abs(u) ** 3) ** 3)
        A = np.vander(u, degree + 1, increasing=True) * sw[:, None]
        fit[i] = np.linalg.lstsq(A, ys[lo:lo + q] * sw, rcond=None)[0][0]
    out = np.empty(m)
    out[order] = fit
    return out


def top_features(variance_standardized, nfeatures: int) -> np.ndarray:
    """Indices of the ``nfeatures`` largest values, descending, by a stable sort: the lower index wins a tie."""
    v = np.asarray(variance_standardized, dtype=np.float64)
    if v.ndim != 1 or np.isnan(v).any():
        raise ValueError("variance_standardized must be a 1-d array without NaN")
    nfeatures = int(nfeatures)
    if nfeatures < 1 or nfeatures > len(v):
        raise ValueError("nfeatures must lie in [1, %d] (got %d)" % (len(v), nfeatures))
    return np.argsort(-v, kind="stable")[:nfeatures].astype(np.int32)


def expected_sd_from_stats(mean, variance, span: float = 0.3) -> np.ndarray:
    """``vst``'s expected standard deviation: ``sqrt(10 ^ loess(log10 variance ~ log10 mean))`` over the genes whose
    variance is not 0, and 0 for those."""
    mean, variance = np.asarray(mean, dtype=np.float64), np.asarray(variance, dtype=np.float64)
    ok = variance > 0
    sd = np.zeros(len(mean))
    if ok.any():
        sd[ok] = np.sqrt(10.0 ** loess_fit(np.log10(mean[ok]), np.log10(variance[ok]), span=span, degree=2))
    return sd


def find_variable_features(X_or_handle, nfeatures: int = 2000, span: float = 0.3, clip_max: Optional[float] = None,
                           expected_sd=None, device: int = 0) -> Result:
    """Seurat's ``FindVariableFeatures(selection.method = "vst")`` on the counts: per-gene mean and variance (device), the
    loess curve of log10 variance on log10 mean over the non-constant genes (host, :func:`loess_fit`; see there what is
    unpinned against R) unless ``expected_sd`` is given, the variance of the values standardised by it and clipped at
    ``clip_max`` (default ``sqrt(n)``; device), and the top ``nfeatures`` by :func:`top_features`.  Returns ``mean``,
    ``variance``, ``variance_expected``, ``variance_standardized`` and ``genes`` (in rank order)."""
    if not isinstance(X_or_handle, ExpressionMatrix):
        with ExpressionMatrix(X_or_handle, device=device) as m:
            return find_variable_features(m, nfeatures, span, clip_max, expected_sd)
    m = X_or_handle
    nfeatures = int(nfeatures)
    if nfeatures < 1 or nfeatures > m.g:
        raise ValueError("nfeatures must lie in [1, %d] (got %d)" % (m.g, nfeatures))
    mean, var, _ = m.gene_stats("counts")
    t0 = time.perf_counter()
    if expected_sd is None:
        sd = expected_sd_from_stats(mean, var, span)
    else:
        sd = np.asarray(expected_sd, dtype=np.float64)
        if sd.shape != (m.g,):
            raise ValueError("expected_sd must have one entry per gene (%d)" % m.g)
    m.timing["loess_s"] = time.perf_counter() - t0
    clip = math.sqrt(m.n) if clip_max is None else float(clip_max)
    vs = m.clipped_variance(mean, sd, clip)
    return Result(mean=mean, variance=var, variance_expected=sd ** 2, variance_standardized=vs,
                  genes=top_features(vs, nfeatures))


def feature_mask(gene_names, pattern: str = "^MT-") -> np.ndarray:
    """Booleans, one per gene: does ``re.search(pattern, name)`` match (case-sensitive, as R's ``grep`` in
    ``PercentageFeatureSet(pattern = ...)``)."""
    rx = re.compile(pattern)
    return np.array([rx.search(str(name)) is not None for name in gene_names], dtype=bool)


def cell_qc(X_or_handle, gene_names=None, pattern: str = "^MT-", mask=None, device: int = 0) -> Result:
    """Seurat's per-cell QC columns of the counts: ``n_count`` (``nCount_RNA``, fp64), ``n_feature`` (``nFeature_RNA``) and
    ``percent`` = ``100 * (total of the gene subset) / n_count`` in host fp64 (``PercentageFeatureSet``), the subset being
    ``mask`` (g booleans) or else the genes whose name matches ``pattern`` (:func:`feature_mask`); ``percent`` is ``None``
    when neither ``mask`` nor ``gene_names`` is given.  A cell without counts gets ``percent`` 0 (Seurat gives NaN there;
    :meth:`ExpressionMatrix.normalize` follows the same convention)."""
    if not isinstance(X_or_handle, ExpressionMatrix):
        with ExpressionMatrix(X_or_handle, device=device) as m:
            return cell_qc(m, gene_names, pattern, mask)
    m = X_or_handle
    if mask is None and gene_names is not None:
        if len(gene_names) != m.g:
            raise ValueError("gene_names must name every gene (%d, got %d)" % (m.g, len(gene_names)))
        mask = feature_mask(gene_names, pattern)
    n_count, n_feature, subset = m.cell_qc(mask)
    percent = None
    if subset is not None:
        percent = np.where(n_count > 0, 100.0 * subset / np.where(n_count > 0, n_count, 1.0), 0.0)
    return Result(n_count=n_count, n_feature=n_feature, percent=percent)


def qc_filter(qc, min_features=200, max_features=2500, max_percent=5.0, min_counts=None, max_counts=None) -> np.ndarray:
    """The cells the notebooks' ``subset(x, nFeature_RNA > 200 & nFeature_RNA < 2500 & percent.mt < 5)`` keeps, as a boolean
    mask: every inequality is strict, ``None`` disables a bound.  ``qc``: the result of :func:`cell_qc`."""
    keep = np.ones(len(qc["n_feature"]), dtype=bool)
    if max_percent is not None and qc["percent"] is None:
        raise ValueError("max_percent needs qc.percent: give cell_qc gene names or a mask, or pass max_percent=None")
    for values, lo, hi in ((qc["n_feature"], min_features, max_features), (qc["n_count"], min_counts, max_counts),
                           (qc["percent"], None, max_percent)):
        if lo is not None:
            keep &= np.asarray(values) > lo
        if hi is not None:
            keep &= np.asarray(values) < hi
    return keep


def design_basis(covariates, n: Optional[int] = None):
    """``(Q, R)`` of the design matrix ``[1, covariates]`` (``numpy.linalg.qr``, fp64): ``Q`` (n, 1 + p) is the orthonormal
    basis :meth:`ExpressionMatrix.select_regressed` takes, ``R`` turns its coefficients into those of the design
    (:func:`regression_betas`).  ``covariates``: (n,) or (n, p) with ``p <= MAX_COVARIATES``, finite.  ``ValueError`` for a
    length other than ``n`` (when given), a non-finite value, too many columns, and a rank-deficient design -- a constant
    covariate or collinear columns: some ``|R_kk| <= n 2^-52 max |R_kk|``."""
    A = np.asarray(covariates, dtype=np.float64)
    if A.ndim == 1:
        A = A[:, None]
    if A.ndim != 2 or A.shape[0] < 2 or A.shape[1] < 1:
        raise ValueError("covariates must be (n,) or (n, p) with n >= 2, p >= 1 (got shape %s)" % (A.shape,))
    if n is not None and A.shape[0] != int(n):
        raise ValueError("covariates must have one row per cell (%d, got %d)" % (int(n), A.shape[0]))
    if A.shape[1] > MAX_COVARIATES:
        raise ValueError("%d covariates exceed %d" % (A.shape[1], MAX_COVARIATES))
    if not np.isfinite(A).all():
        raise ValueError("covariates must be finite")
    if A.shape[0] < A.shape[1] + 1:
        raise ValueError("%d cells cannot carry a design of %d columns" % (A.shape[0], A.shape[1] + 1))
    const = np.flatnonzero(A.min(axis=0) == A.max(axis=0))
    if len(const):
        raise ValueError("covariate %d is constant: the design is rank-deficient" % const[0])
    Q, R = np.linalg.qr(np.column_stack([np.ones(A.shape[0]), A]))
    d = np.abs(np.diag(R))
    if (d <= A.shape[0] * 2.0 ** -52 * d.max()).any():
        raise ValueError("the design [1, covariates] is rank-deficient (column %d depends on those before it)"
                         % int(np.argmin(d)))
    return np.ascontiguousarray(Q), R


def regression_betas(R, coef_q) -> np.ndarray:
    """The coefficients of the design ``[1, covariates]`` from those of its basis: ``beta = R^-1 c`` (row 0 the intercept,
    then one row per covariate; one column per gene)."""
    from scipy.linalg import solve_triangular
    return solve_triangular(np.asarray(R, dtype=np.float64), np.asarray(coef_q, dtype=np.float64), lower=False)


def _select_scaled(m: ExpressionMatrix, genes, max_value: float, vars_to_regress=None):
    """-> the ``regression`` table when ``vars_to_regress`` is given, else ``None``"""
    genes = np.asarray(genes)
    if genes.ndim != 1 or genes.dtype.kind not in "iu" or len(genes) < 1:
        raise ValueError("genes must be a non-empty 1-d integer array")
    if genes.min() < 0 or genes.max() >= m.g:
        raise ValueError("gene indices must lie in [0, %d)" % m.g)
    if vars_to_regress is None:
        mean, var, _ = m.gene_stats("normalized")
        m.select(genes, mean[genes], np.sqrt(var[genes]), max_value)
        return None
    t0 = time.perf_counter()
    Q, R = design_basis(vars_to_regress, n=m.n)
    m.timing["design_qr_s"] = time.perf_counter() - t0
    m.select_regressed(genes, Q, max_value)
    return Result(betas=regression_betas(R, m.coef_q), resid_mean=m.resid_mean, resid_var=m.resid_var, flat=m.flat)


def scale_data(handle: ExpressionMatrix, genes, max_value: float = 10.0, vars_to_regress=None) -> np.ndarray:
    """Seurat's ``ScaleData`` on the chosen genes of the normalised matrix: centred by the gene's mean, divided by its
    standard deviation (ddof 1), clipped above at ``max_value``; a constant gene gives zeros.  Returns ``Z`` (n x h, fp32).
    ``vars_to_regress`` ((n,) or (n, p <= 8) covariates, e.g. ``cell_qc(...).percent``): Seurat's ``vars.to.regress`` with
    its default linear model -- per gene the residuals of ``y ~ 1 + covariates`` are centred, scaled and clipped instead
    (:meth:`ExpressionMatrix.select_regressed`), and ``handle.regression`` holds ``betas`` (:func:`regression_betas`),
    ``resid_mean``, ``resid_var`` and ``flat``."""
    handle.regression = _select_scaled(handle, genes, max_value, vars_to_regress)
    return handle.fetch_scaled()


def pca_from_gram(G, n: int, npcs: int) -> Result:
    """The top ``npcs`` eigenpairs of ``G / (n - 1)`` (``scipy.linalg.eigh``, fp64), descending.  Each loading's sign makes
    its largest-magnitude entry positive (the first such entry on ties) -- a convention of this package: irlba's signs, which
    Seurat reports, are arbitrary and UNPINNED.  Returns ``loadings`` (h x npcs), ``eigenvalues``, ``stdev`` (their square
    roots, Seurat's ``stdev``) and ``total_variance`` (trace / (n - 1))."""
    from scipy.linalg import eigh
    G = np.asarray(G, dtype=np.float64)
    if G.ndim != 2 or G.shape[0] != G.shape[1]:
        raise ValueError("G must be square")
    h, n, npcs = G.shape[0], int(n), int(npcs)
    if n < 2:
        raise ValueError("n must be at least 2")
    if npcs < 1 or npcs > h:
        raise ValueError("npcs must lie in [1, %d] (got %d)" % (h, npcs))
    Cm = G / (n - 1.0)
    w, V = eigh(Cm, subset_by_index=[h - npcs, h - 1])
    w, V = w[::-1].copy(), V[:, ::-1].copy()
    top = np.argmax(np.abs(V), axis=0)                           # (argmax: the first of equal magnitudes)
    V *= np.where(V[top, np.arange(npcs)] < 0, -1.0, 1.0)
    return Result(loadings=V, eigenvalues=w, stdev=np.sqrt(np.maximum(w, 0.0)), total_variance=float(np.trace(Cm)))


def pca(handle: ExpressionMatrix, genes, npcs: int = 50, max_value: float = 10.0, vars_to_regress=None) -> Result:
    """Seurat's ``ScaleData`` + ``RunPCA(features = genes)``: the scaled matrix, its Gram matrix (device),
    :func:`pca_from_gram` (host), and ``coords = Z @ f32(loadings)`` (device): Seurat's ``cell.embeddings``.  Returns the
    fields of :func:`pca_from_gram`, ``coords`` (n x npcs, fp32) and ``timing`` (every kernel's ms, the eigen-solve's
    seconds).  With ``vars_to_regress`` (see :func:`scale_data`) the scaled matrix is that of the residuals and
    ``regression`` (``betas``, ``resid_mean``, ``resid_var``, ``flat``) is returned as well."""
    npcs = int(npcs)
    if npcs < 1 or npcs > min(MAX_PCS, len(np.atleast_1d(genes))):
        raise ValueError("npcs must lie in [1, min(%d, number of genes)] (got %d)" % (MAX_PCS, npcs))
    regression = _select_scaled(handle, genes, max_value, vars_to_regress)
    G = handle.gram()
    t0 = time.perf_counter()
    r = pca_from_gram(G, handle.n, npcs)
    handle.timing["eigh_s"] = time.perf_counter() - t0
    r["coords"] = handle.project(r.loadings.astype(np.float32))
    r["timing"] = dict(handle.timing)
    if regression is not None:
        r["regression"] = regression
    return r


def embed(X, nfeatures: int = 2000, npcs: int = 50, scale_factor: float = 1e4, max_value: float = 10.0, span: float = 0.3,
          device: int = 0, vars_to_regress=None) -> Result:
    """The whole chain on one upload: normalise, ``vst`` variable genes, scale, PCA.  Returns the fields of :func:`pca`
    plus ``genes`` and ``features`` (the table of :func:`find_variable_features`).  ``coords[:, :dim]`` is what
    :func:`snn.build_snn` takes.  ``X`` is dense or ``scipy.sparse`` (the same genes and coordinates either way).
    ``vars_to_regress``: one row per cell of ``X``, regressed out of the chosen genes before scaling (see
    :func:`scale_data`).  For ``SCTransform`` see :func:`sctransform`."""
    with ExpressionMatrix(X, device=device) as m:
        m.normalize(scale_factor)
        feats = find_variable_features(m, nfeatures=nfeatures, span=span)
        r = pca(m, feats.genes, npcs=npcs, max_value=max_value, vars_to_regress=vars_to_regress)
    r["genes"] = feats.genes
    r["features"] = feats
    return r


# ---- SCTransform -----------------------------------------------------------------------------------------------------------
# A specification of this package, modelled on sctransform::vst as Seurat's SCTransform calls it; R is not available to
# compare against and its sub-sampling draws from R's generator, so agreement with R is UNPINNED.

SCT_MAX_FIT_CELLS = 8192   # MI_PREP_SCT_MAX_FIT_CELLS
_EPS = 2.0 ** -52


def sct_cell_subsample(n: int, ncells: int = 5000, seed: int = 0) -> np.ndarray:
    """The cells of step 1: all when ``n <= ncells``, else ``ncells`` drawn without replacement
    (``default_rng(seed).choice``), sorted."""
    n, ncells = int(n), int(ncells)
    if ncells < 3:
        raise ValueError("ncells must be at least 3")
    if n <= ncells:
        return np.arange(n, dtype=np.int32)
    return np.sort(np.random.default_rng(seed).choice(n, ncells, replace=False)).astype(np.int32)


def _bw_nrd(x) -> float:
    q75, q25 = np.percentile(x, [75, 25])
    return 1.06 * min(np.std(x, ddof=1), (q75 - q25) / 1.34) * len(x) ** -0.2


def _gauss_density(x, bw, block=2048) -> np.ndarray:
    """the Gaussian kernel density estimate of the sample ``x`` at its own points, evaluated directly"""
    out = np.empty(len(x))
    for s in range(0, len(x), block):
        u = (x[s:s + block, None] - x[None, :]) / bw
        out[s:s + block] = np.exp(-0.5 * u * u).sum(axis=1)
    return out / (len(x) * bw * math.sqrt(2.0 * math.pi))


def sct_gene_subsample(log_gmean, n_genes: int = 2000, seed: int = 0) -> np.ndarray:
    """The genes of step 1, as positions in ``log_gmean``: all when at most ``n_genes``, else ``n_genes`` drawn without
    replacement with probability proportional to ``1 / (density(log_gmean) + 2^-52)`` (a Gaussian kernel estimate with the
    bandwidth ``1.06 min(sd, IQR / 1.34) G^(-1/5)``; ``default_rng([1, seed])``), sorted: sctransform's way of covering
    the range of expression evenly."""
    x = np.asarray(log_gmean, dtype=np.float64)
    n_genes = int(n_genes)
    if x.ndim != 1 or not np.isfinite(x).all():
        raise ValueError("log_gmean must be a finite 1-d array")
    if n_genes < 1:
        raise ValueError("n_genes must be at least 1")
    if len(x) <= n_genes:
        return np.arange(len(x), dtype=np.int64)
    bw = _bw_nrd(x)
    w = 1.0 / (_gauss_density(x, bw if bw > 0 else 1.0) + _EPS)
    return np.sort(np.random.default_rng([1, int(seed)]).choice(len(x), n_genes, replace=False, p=w / w.sum()))


def _sj_functionals(x):
    """-> (n, scale, SD(h), TD(h)) of Sheather and Jones: the estimates of the integrated squared second and third
    derivative of the density from all pairs (diagonal included), unbinned"""
    n = len(x)
    iu = np.triu_indices(n, 1)
    d2 = (x[iu[0]] - x[iu[1]]) ** 2
    q75, q25 = np.percentile(x, [75, 25])
    scale = min(np.std(x, ddof=1), (q75 - q25) / 1.349)
    root2pi = math.sqrt(2.0 * math.pi)

    def SD(h):
        t = d2 / (h * h)
        s = (np.exp(-0.5 * t) * (t * t - 6.0 * t + 3.0)).sum()
        return (2.0 * s + 3.0 * n) / (n * (n - 1.0) * h ** 5 * root2pi)

    def TD(h):
        t = d2 / (h * h)
        s = (np.exp(-0.5 * t) * (t * t * t - 15.0 * t * t + 45.0 * t - 15.0)).sum()
        return -(2.0 * s - 15.0 * n) / (n * (n - 1.0) * h ** 7 * root2pi)

    return n, scale, SD, TD


def bw_sj(x, rtol: float = 1e-10) -> float:
    """The Sheather-Jones "solve-the-equation" bandwidth of a Gaussian kernel density estimate (R's ``bw.SJ``), by direct
    evaluation over all pairs and bisection: the root ``h`` of ``(1 / (2 sqrt(pi) n SD(alpha2 h^(5/7))))^(1/5) = h`` with
    ``alpha2 = 1.357 (SD(a) / TD(b))^(1/7)``, ``a = 1.24 s n^(-1/7)``, ``b = 1.23 s n^(-1/9)``, ``s = min(sd, IQR / 1.349)``.
    The bracket starts at R's ``[0.1, 1] * 1.144 s n^(-1/5)`` and widens by 1.2 until the sign changes."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 1 or len(x) < 3 or not np.isfinite(x).all():
        raise ValueError("x must be a finite 1-d array of at least 3 values")
    n, scale, SD, TD = _sj_functionals(x)
    if not scale > 0:
        raise ValueError("x has no spread: the bandwidth is undefined")
    c1 = 1.0 / (2.0 * math.sqrt(math.pi) * n)
    alph2 = 1.357 * (SD(1.24 * scale * n ** (-1.0 / 7.0)) / TD(1.23 * scale * n ** (-1.0 / 9.0))) ** (1.0 / 7.0)
    if not np.isfinite(alph2):
        raise ValueError("the sample is too sparse for the Sheather-Jones bandwidth")

    def f(h):
        return (c1 / SD(alph2 * h ** (5.0 / 7.0))) ** 0.2 - h

    hi = 1.144 * scale * n ** -0.2
    lo = 0.1 * hi
    flo, fhi = f(lo), f(hi)
    for _ in range(100):
        if flo * fhi <= 0:
            break
        lo, hi = lo / 1.2, hi * 1.2
        flo, fhi = f(lo), f(hi)
    else:
        raise ValueError("no solution of the Sheather-Jones equation was bracketed")
    while hi - lo > rtol * hi:
        mid = 0.5 * (lo + hi)
        fm = f(mid)
        if flo * fm <= 0:
            hi = mid
        else:
            lo, flo = mid, fm
    return 0.5 * (lo + hi)


def kernel_smooth(x, y, x_out, bandwidth: float, block: int = 2048) -> np.ndarray:
    """Nadaraya-Watson with a normal kernel in R's ``ksmooth`` scaling: the kernel's sd is ``0.3706506 * bandwidth`` (its
    quartiles at ``+-bandwidth / 4``), truncated at 4 sd.  ``y``: (m,) or (m, k).  NaN where no point lies in reach."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    xo = np.asarray(x_out, dtype=np.float64)
    sd = 0.3706506 * float(bandwidth)
    if not sd > 0:
        raise ValueError("bandwidth must be > 0")
    y2 = y if y.ndim == 2 else y[:, None]
    out = np.empty((len(xo), y2.shape[1]))
    for s in range(0, len(xo), block):
        d = xo[s:s + block, None] - x[None, :]
        w = np.where(np.abs(d) <= 4.0 * sd, np.exp(-0.5 * (d / sd) ** 2), 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[s:s + block] = (w @ y2) / w.sum(axis=1)[:, None]
    return out if y.ndim == 2 else out[:, 0]


def _binned_robust_score(v, x, lo, width):
    b = np.floor((x - lo) / width).astype(np.int64)
    score = np.zeros(len(v))
    for k in np.unique(b):
        sel = b == k
        med = np.median(v[sel])
        mad = 1.4826 * np.median(np.abs(v[sel] - med))
        score[sel] = (v[sel] - med) / (mad + _EPS)
    return score


def sct_outliers(values, x, threshold: float = 10.0) -> np.ndarray:
    """sctransform's ``is_outlier``: the robust z-score ``(v - median) / (1.4826 MAD + 2^-52)`` within bins of ``x`` of
    width ``(max - min) bw_sj(x) / 2``, on two grids offset by half a bin; an outlier exceeds ``threshold`` in absolute
    value on both."""
    v, x = np.asarray(values, dtype=np.float64), np.asarray(x, dtype=np.float64)
    width = (x.max() - x.min()) * bw_sj(x) / 2.0
    s1 = _binned_robust_score(v, x, x.min(), width)
    s2 = _binned_robust_score(v, x, x.min() - 0.5 * width, width)
    return np.minimum(np.abs(s1), np.abs(s2)) > threshold


def sct_regularize(log_gmean_fit, b0, b1, alpha, log_gmean_all, bw_adjust: float = 3.0, threshold: float = 10.0) -> Result:
    """sctransform's ``reg_model_pars``, host fp64.  The fitted ``alpha`` becomes the overdispersion factor
    ``od = log10(1 + 10^log_gmean alpha)`` (0 for a Poisson gene); genes that are outliers (:func:`sct_outliers`, or a
    non-finite parameter) in ``b0``, ``b1`` or ``od`` are dropped; the three are smoothed over ``log_gmean`` by
    :func:`kernel_smooth` with ``bandwidth = bw_adjust * bw_sj(log_gmean of the kept genes)`` and evaluated at every gene of
    ``log_gmean_all``, clamped to the range of the kept genes; ``alpha = (10^od - 1) / 10^log_gmean``.  Returns ``b0``,
    ``b1``, ``alpha``, ``od`` (per gene of ``log_gmean_all``), ``outlier`` (per fitted gene) and ``bandwidth``."""
    x = np.asarray(log_gmean_fit, dtype=np.float64)
    par = np.column_stack([np.asarray(a, dtype=np.float64) for a in (b0, b1, alpha)])
    xa = np.asarray(log_gmean_all, dtype=np.float64)
    if x.ndim != 1 or par.shape != (len(x), 3) or len(x) < 3:
        raise ValueError("log_gmean_fit, b0, b1 and alpha must be 1-d arrays of one length >= 3")
    if not (np.isfinite(x).all() and np.isfinite(xa).all()):
        raise ValueError("log_gmean must be finite")
    bad = ~np.isfinite(par).all(axis=1) | (par[:, 2] < 0)
    par = np.where(bad[:, None], 0.0, par)
    par[:, 2] = np.log10(1.0 + 10.0 ** x * par[:, 2])
    outlier = bad.copy()
    ok = ~bad
    for k in range(3):
        outlier[ok] |= sct_outliers(par[ok, k], x[ok], threshold)
    keep = ~outlier
    if keep.sum() < 3:
        raise ValueError("fewer than 3 fitted genes are left to regularise")
    bw = float(bw_adjust) * bw_sj(x[keep])
    xs = np.clip(xa, x[keep].min(), x[keep].max())
    sm = kernel_smooth(x[keep], par[keep], xs, bw)
    return Result(b0=sm[:, 0], b1=sm[:, 1], od=sm[:, 2], alpha=np.maximum(10.0 ** sm[:, 2] - 1.0, 0.0) / 10.0 ** xa,
                  outlier=outlier, bandwidth=bw)


def _detected_in(X, cells) -> np.ndarray:
    """cells with a non-zero count per gene among ``cells`` (host)"""
    if is_sparse(X):
        return np.asarray((X.tocsr()[cells] != 0).sum(axis=0)).ravel()
    return (np.asarray(X)[cells] != 0).sum(axis=0)


def sctransform(X, variable_features_n: int = 3000, npcs: int = 50, vars_to_regress=None, ncells: int = 5000,
                n_genes: int = 2000, min_cells: int = 5, seed: int = 0, clip: Optional[float] = None, device: int = 0,
                cells=None, genes=None, return_corrected: bool = False) -> Result:
    """Seurat's ``SCTransform(vars.to.regress = ...)`` + ``RunPCA(features = VariableFeatures)`` on one upload, as this
    package specifies it (unpinned against R): per-cell ``log_umi = log10(total)`` and per-gene ``detected`` and
    ``log_gmean`` (device); the step-1 sub-samples (:func:`sct_cell_subsample`, :func:`sct_gene_subsample`; ``cells=`` and
    ``genes=`` override them); the per-gene negative-binomial regression on ``log_umi`` (device,
    :meth:`ExpressionMatrix.nb_fit`); :func:`sct_regularize` (host); the variance of the Pearson residuals of every gene
    detected in ``min_cells`` cells, clipped at ``sqrt(n)`` (device), whose top ``variable_features_n`` are the variable
    features; their residuals clipped at ``clip`` (default ``sqrt(n / 30)``), centred and, with ``vars_to_regress``,
    regressed (device, :meth:`ExpressionMatrix.select_pearson`); Gram matrix, eigen-solve, projection as :func:`pca`.

    Returns the fields of :func:`pca` plus ``genes`` (rank order), ``gene_attr`` (per gene of ``X``: ``detected``,
    ``log_gmean``, ``passing``, the regularised ``b0``, ``b1``, ``alpha`` and ``residual_mean`` / ``residual_variance``,
    NaN where not passing), ``model`` (the step-1 table: ``genes``, ``cells``, the fields of ``nb_fit``, ``outlier``),
    ``log_umi`` and ``timing``.  ``ValueError`` for a cell without counts: run :func:`qc_filter` first.

    ``return_corrected=True`` adds ``corrected``, an OPEN :class:`ExpressionMatrix` of the kind and shape of ``X`` that the
    caller closes: the corrected counts (``fetch_counts()``) and the ``data`` slot ``log1p`` of them (``fetch_normalized()``;
    the matrix ``find_all_markers(r.corrected, labels)`` ranks and ``cluster_stats(r.corrected.fetch_normalized(), labels)``
    takes) of the ``passing`` genes under their regularised parameters at the depth ``log10(median(n_count))``
    (:meth:`ExpressionMatrix.sct_correct`), and ``median_umi``.  Every gene of ``X`` keeps its column, all zero where it is
    not passing -- a convention of this package: Seurat keeps the passing genes alone.  Without the flag the call is what
    it was: the same outputs, passes and timing keys.

    Not built: ``vst.flavor = "v2"``, ``batch_var``, a corrected matrix restricted to Seurat's gene subset, agreement with R
    (unpinned throughout), latent variables other than ``log_umi``, glmGamPoi's Cox-Reid adjustment, more than
    ``MAX_FEATURES`` features."""
    with ExpressionMatrix(X, device=device) as m:
        n = m.n
        n_count, _, _ = m.cell_qc()
        if (n_count <= 0).any():
            raise ValueError("cell %d has no counts: SCTransform needs log10 of every cell's total (run qc_filter first)"
                             % int(np.flatnonzero(n_count <= 0)[0]))
        log_umi = np.log10(n_count)
        _, _, detected = m.gene_stats("counts")
        log_gmean = np.full(m.g, -np.inf)
        with np.errstate(divide="ignore"):
            log_gmean = np.log10(np.expm1(m.gene_log1p_sum() / n))
        passing = np.flatnonzero(detected >= int(min_cells)).astype(np.int32)
        if len(passing) < 3:
            raise ValueError("fewer than 3 genes are detected in %d cells" % int(min_cells))
        t0 = time.perf_counter()
        cells = sct_cell_subsample(n, min(int(ncells), SCT_MAX_FIT_CELLS), seed) if cells is None else np.asarray(cells)
        if genes is None:
            cand = passing if len(cells) == n else passing[_detected_in(X, cells)[passing] >= int(min_cells)]
            genes = cand[sct_gene_subsample(log_gmean[cand], min(int(n_genes), MAX_FEATURES), seed)]
        genes = np.asarray(genes)
        m.timing["sct_subsample_s"] = time.perf_counter() - t0
        fit = m.nb_fit(cells, genes, log_umi[cells])
        t0 = time.perf_counter()
        reg = sct_regularize(log_gmean[genes], fit.b0, fit.b1, fit.alpha, log_gmean[passing])
        m.timing["sct_regularize_s"] = time.perf_counter() - t0
        rmean, rvar = m.sct_residual_moments(passing, reg.b0, reg.b1, reg.alpha, log_umi)
        top = top_features(rvar, min(int(variable_features_n), len(passing), MAX_FEATURES))
        feats = passing[top]
        npcs = int(npcs)
        if npcs < 1 or npcs > min(MAX_PCS, len(feats)):
            raise ValueError("npcs must lie in [1, min(%d, number of features)] (got %d)" % (MAX_PCS, npcs))
        Q = R = None
        if vars_to_regress is not None:
            Q, R = design_basis(vars_to_regress, n=n)
        m.select_pearson(feats, reg.b0[top], reg.b1[top], reg.alpha[top], log_umi, Q=Q, clip=clip)
        G = m.gram()
        t0 = time.perf_counter()
        r = pca_from_gram(G, n, npcs)
        m.timing["eigh_s"] = time.perf_counter() - t0
        r["coords"] = m.project(r.loadings.astype(np.float32))
        if R is not None:
            r["regression"] = Result(betas=regression_betas(R, m.coef_q), resid_mean=m.resid_mean, resid_var=m.resid_var,
                                     flat=m.flat)
        if return_corrected:
            median_umi = float(np.median(n_count))
            r["corrected"] = m.sct_correct(passing, reg.b0, reg.b1, reg.alpha, log_umi, math.log10(median_umi))
            r["median_umi"] = median_umi
        r["timing"] = dict(m.timing)
    attr = Result(detected=detected, log_gmean=log_gmean, passing=np.isin(np.arange(len(detected)), passing))
    for name, values in (("b0", reg.b0), ("b1", reg.b1), ("alpha", reg.alpha), ("residual_mean", rmean),
                         ("residual_variance", rvar)):
        attr[name] = np.full(len(detected), np.nan)
        attr[name][passing] = values
    r["genes"] = feats
    r["gene_attr"] = attr
    r["model"] = Result(fit, genes=genes, cells=np.asarray(cells), outlier=reg.outlier, bandwidth=reg.bandwidth)
    r["log_umi"] = log_umi
    return r


def _first_existing(path, names):
    for name in names:
        f = os.path.join(path, name)
        if os.path.exists(f):
            return f
    raise FileNotFoundError("%s holds none of %s" % (path, ", ".join(names)))


def _read_tsv(f):
    import gzip
    with (gzip.open(f, "rt") if f.endswith(".gz") else open(f)) as fh:
        return [line.rstrip("\r\n").split("\t") for line in fh if line.strip()]


def read_10x_mtx(path):
    """A 10x Genomics matrix directory -- ``matrix.mtx`` (genes x cells, Matrix Market), ``genes.tsv`` (id, name) or
    ``features.tsv`` (id, name, type) and ``barcodes.tsv``, each plain or ``.gz`` -- as ``(counts, barcodes, gene_ids,
    gene_names)``: counts a cells x genes ``csr_matrix`` of float32 (``scipy.io.mmread``, transposed), the three lists in
    file order.  Host only."""
    from scipy.io import mmread
    M = mmread(_first_existing(path, ("matrix.mtx", "matrix.mtx.gz")))
    genes = _read_tsv(_first_existing(path, ("genes.tsv", "genes.tsv.gz", "features.tsv", "features.tsv.gz")))
    barcodes = [row[0] for row in _read_tsv(_first_existing(path, ("barcodes.tsv", "barcodes.tsv.gz")))]
    if not is_sparse(M):
        raise ValueError("matrix.mtx must be a coordinate (sparse) Matrix Market file")
    counts = M.T.tocsr().astype(np.float32)
    counts.sum_duplicates()
    if counts.shape != (len(barcodes), len(genes)):
        raise ValueError("matrix.mtx is %d genes x %d cells, the lists name %d genes and %d cells"
                         % (counts.shape[1], counts.shape[0], len(genes), len(barcodes)))
    return counts, barcodes, [row[0] for row in genes], [row[1] if len(row) > 1 else row[0] for row in genes]
