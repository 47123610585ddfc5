"""SCTransform on the device (``mi_prep_gene_log1p_sum``, ``mi_prep_nb_fit``, ``mi_prep_sct_residual_moments``,
``mi_prep_sct_select``, ``preprocess.sctransform``) against the numpy fp64 restatement of tests/sct_reference.py.

The fit.  Shapes are the kernel's edges: one, two and many cells per thread (m = 64, 255, 256, 257, 600), the LDS limit
(m = 8192, 8 genes), G1 = 1, 63, 65 and all genes of an input; one case fits a shuffled subset of the cells and genes of a
larger handle.  ``poisson`` and ``converged`` equal the restatement's.  ``iterations`` is compared to +-1: the stopping
number of a gene in its last rounds lies near 1e-16, and the restatement itself changes a count by one on some gene when the
cells are permuted (seen at (600, 256, 1) and (257, 130, 2)); nothing else is loosened.  ``b0c``, ``b1`` and ``alpha`` agree
within TAU standard errors, TAU = 100 x the restatement's own sensitivity to the order of summation (its largest change, in
standard errors, over three permutations of the cells of each of the three inputs of ``sct_cases.FIT_CASES``).  MEASURED:
sensitivity 2.9e-8 se, so TAU = 2.9e-6 (the condition TAU <= 1e-3 holds with three decades to spare); on an MI355X the
device's largest deviation from the restatement over all shapes is 2.8e-8 se (m = 257; 2.4e-11 at m = 8192) and the stopping
number evaluated on the host at the device's parameters at most 1.1e-8 (``test_fit_matches_the_restatement`` prints both;
DESIGN.md section 5c "SCTransform").  Every gene here converges; genes at the round limit, failed fits, the alpha bounds, the
Poisson rule's edge and counts of 2^24 are tests/test_gpu_sct_edges.py.

Residual moments: variance within the project's RTOL about the device's own mean, mean within 1e-9 sum |r| / n.  Z: stage 1
within 2^-24 |ref| + 1e-12 (x + mu) / sigma of the fp64 expression; stages 2 - 5 bit for bit the numpy expression of
tests/prep_regress_cases.py at unit scale from the device's stage-1 matrix and coefficients; columns orthogonal to the design
within 2 * 2^-24 |z_j| (each z carries one f32 rounding, |q_k| = 1, a margin of 2).  Sparse against dense and run against run:
``np.array_equal`` on every output of every entry."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import prep_reference as ref
import prep_regress_cases as rc
import sct_cases as sc
import sct_reference as sr
from scrna_seq_qannealing_clustering_amd import _lib, preprocess, snn
from scrna_seq_qannealing_clustering_amd.preprocess import ExpressionMatrix

pytestmark = pytest.mark.gpu

RTOL = 1e-9                                   # the project's fp64 tolerance (tests/test_gpu_prep.py)
EINVAL, EUNSUPPORTED, ESTATE = -1, -5, -6
FIT_KEYS = ("b0", "b1", "alpha", "se_b0c", "se_b1", "se_alpha", "iterations", "converged", "poisson")


@functools.lru_cache(maxsize=None)
def tau():
    """100 x the restatement's sensitivity to the order of summation, in standard errors"""
    worst = 0.0
    for case in sc.FIT_CASES:
        d = sc.nb_counts(*case)
        f = sr.nb_fit(d["Y"], d["log_umi"])
        for k in range(3):
            perm = np.random.default_rng(100 + k).permutation(len(d["log_umi"]))
            f2 = sr.nb_fit(d["Y"][perm], d["log_umi"][perm])
            assert np.array_equal(f2["poisson"], f["poisson"])
            for key, se in (("b0c", "se_b0c"), ("b1", "se_b1"), ("alpha", "se_alpha")):
                worst = max(worst, float(np.nanmax(np.abs(f2[key] - f[key]) / f[se])))
    print("restatement sensitivity %.3g se -> tau %.3g" % (worst, 100 * worst))
    return 100.0 * worst


# (cells, genes drawn, seed of sct_cases.nb_counts, genes used or None for all)
FIT_SHAPES = [(64, 130, 4, None), (255, 130, 6, None), (256, 130, 7, None), (257, 130, 2, None), (600, 256, 1, None),
              (8192, 12, 5, 8), (257, 130, 2, 1), (257, 130, 2, 63), (257, 130, 2, 65)]


@functools.lru_cache(maxsize=None)
def fit_case(m, G, seed, g1):
    d = sc.nb_counts(m, G, seed)
    Y = d["Y"] if g1 is None else d["Y"][:, :g1]
    with ExpressionMatrix(Y) as h:
        dev = h.nb_fit(np.arange(m), np.arange(Y.shape[1]), d["log_umi"])
        assert h.timing["nb_fit_ms"] >= 0.0
    return d, Y, dev, sr.nb_fit(Y, d["log_umi"])


def assert_fit_matches(dev, want, Y, log_umi):
    assert want["converged"].all()                               # (the condition of the comparison)
    assert np.array_equal(dev.poisson, want["poisson"]) and np.array_equal(dev.converged, want["converged"])
    assert np.abs(dev.iterations.astype(int) - want["iterations"]).max() <= 1
    b0c = dev.b0 + dev.b1 * dev.log_umi_mean
    t = tau()
    assert t <= 1e-3
    worst = 0.0
    for got, key, se in ((b0c, "b0c", "se_b0c"), (dev.b1, "b1", "se_b1"), (dev.alpha, "alpha", "se_alpha")):
        dz = np.abs(got - want[key]) / want[se]
        dz = np.where(want["poisson"] & (key == "alpha"), np.abs(got - want[key]), dz)       # (alpha = 0 exactly)
        worst = max(worst, float(dz.max()))
    lam = sr.stop_number(Y, log_umi, b0c, dev.b1, dev.alpha, dev.poisson)
    print("device - restatement: %.3g se; host-evaluated lambda at the device's parameters: %.3g; tau %.3g; rounds <= %d"
          % (worst, lam.max(), t, dev.iterations.max()))
    assert worst <= t
    assert lam.max() <= t
    for key in ("se_b0c", "se_b1", "se_alpha"):
        np.testing.assert_allclose(dev[key], want[key], rtol=1e-6, equal_nan=True)
    assert np.isnan(dev.se_alpha[dev.poisson]).all() and (dev.alpha[dev.poisson] == 0).all()


@pytest.mark.parametrize("m,G,seed,g1", FIT_SHAPES)
def test_fit_matches_the_restatement(m, G, seed, g1):
    d, Y, dev, want = fit_case(m, G, seed, g1)
    assert dev.b0.shape == (Y.shape[1],) and dev.iterations.dtype == np.int32 and dev.converged.dtype == np.bool_
    assert_fit_matches(dev, want, Y, d["log_umi"])


def test_fit_of_a_shuffled_subset_of_cells_and_genes():
    d = sc.nb_counts(600, 256, 1)
    rng = np.random.default_rng(11)
    cells, genes = rng.permutation(600)[:257], rng.permutation(d["Y"].shape[1])[:65]
    with ExpressionMatrix(d["Y"]) as h:
        dev = h.nb_fit(cells, genes, d["log_umi"][cells])
    Y = d["Y"][np.ix_(cells, genes)]
    assert_fit_matches(dev, sr.nb_fit(Y, d["log_umi"][cells]), Y, d["log_umi"][cells])


def test_fit_recovers_the_planted_parameters():
    d, _, dev, _ = fit_case(600, 256, 1, None)
    sc.check_recovery(dev, d)


# ---- gene attributes ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,g", [(2, 1), (255, 63), (257, 65), (1027, 150)])
def test_gene_log1p_sum(n, g):
    X = ref.sparse_counts(np.random.default_rng(n + g), n, g)
    with ExpressionMatrix(X) as d, ExpressionMatrix(sp.csr_matrix(X)) as s:
        got, again, sparse = d.gene_log1p_sum(), d.gene_log1p_sum(), s.gene_log1p_sum()
    np.testing.assert_allclose(got, np.log1p(X.astype(np.float64)).sum(axis=0), rtol=RTOL, atol=0.0)
    assert np.array_equal(got, again) and np.array_equal(got, sparse)


# ---- residual moments -----------------------------------------------------------------------------------------------------

def residual_inputs(n, g, seed=0):
    """counts, log_umi (drawn, so that an empty cell has one), plausible parameters; gene 0's largest count is raised until
    its residual passes sqrt(n)"""
    rng = np.random.default_rng(1000 * n + g + seed)
    X = ref.sparse_counts(rng, n, g)
    lu = rng.uniform(2.5, 4.0, n)
    b1 = rng.normal(2.3, 0.3, g)
    b0 = np.log(X.astype(np.float64).mean(axis=0) + 0.1) - b1 * lu.mean()
    alpha = np.where(np.arange(g) % 3 == 0, 0.0, rng.uniform(0.0, 1.0, g))
    X[0, 0] = 50000.0
    return X, lu, b0, b1, alpha


MOMENT_SHAPES = [(n, 65) for n in (2, 255, 256, 257, 1027)] + [(257, g) for g in (1, 63, 150)]


@pytest.mark.parametrize("n,g", MOMENT_SHAPES)
def test_residual_moments(n, g):
    X, lu, b0, b1, alpha = residual_inputs(n, g)
    genes = np.random.default_rng(g).permutation(g)
    with ExpressionMatrix(X) as m:
        mean, var = m.sct_residual_moments(genes, b0[genes], b1[genes], alpha[genes], lu)
    clip = np.sqrt(n)
    r = sr.residuals(X[:, genes], b0[genes], b1[genes], alpha[genes], lu, clip)
    assert r[0, np.flatnonzero(genes == 0)[0]] == clip           # the clip is exercised
    assert np.all(np.abs(mean - r.sum(axis=0) / n) <= 1e-9 * np.abs(r).sum(axis=0) / n)
    np.testing.assert_allclose(var, ((r - mean) ** 2).sum(axis=0) / (n - 1), rtol=RTOL, atol=0.0)
    assert (var > 0).all()


# ---- Z ------------------------------------------------------------------------------------------------------------------------

Z_SHAPES = [(257, h, 2) for h in (1, 63, 64, 65, 128, 129)] + [(257, 65, q) for q in (1, 9)] + [(1027, 65, 2)]
G_Z = 150


@functools.lru_cache(maxsize=None)
def z_case(n, h, q):
    X, lu, b0, b1, alpha = residual_inputs(n, G_Z, seed=7)
    rng = np.random.default_rng(100 * h + q)
    genes = rng.permutation(G_Z)[:h]
    Q = rc.intercept_basis(n) if q == 1 else preprocess.design_basis(rc.covariates(rng, X, q - 1))[0]
    clip = np.sqrt(n / 30.0)
    par = (b0[genes], b1[genes], alpha[genes])
    with ExpressionMatrix(X) as m:
        Z1 = m.select_pearson(genes, *par, lu, center=False).fetch_scaled()
        m.select_pearson(genes, *par, lu, Q=Q)
        out = {"Z": m.fetch_scaled(), "coef_q": m.coef_q, "resid_mean": m.resid_mean, "resid_var": m.resid_var, "flat": m.flat}
        assert m.timing["sct_select_ms"] >= 0.0
    return X[:, genes], lu, par, Q, clip, Z1, out


@pytest.mark.parametrize("n,h,q", Z_SHAPES)
def test_stage_one_is_the_clipped_residual(n, h, q):
    Xg, lu, (b0, b1, alpha), _, clip, Z1, _ = z_case(n, h, q)
    want = sr.residuals(Xg, b0, b1, alpha, lu, clip)
    mu = np.exp(b0[None, :] + b1[None, :] * lu[:, None])
    sigma = np.sqrt(mu + alpha[None, :] * mu * mu)
    assert Z1.shape == (n, h) and Z1.dtype == np.float32
    assert np.all(np.abs(Z1 - want) <= 2.0 ** -24 * np.abs(want) + 1e-12 * (Xg + mu) / sigma)
    assert (np.abs(want) == clip).any() and np.abs(Z1).max() == np.float32(clip)


@pytest.mark.parametrize("n,h,q", Z_SHAPES)
def test_stages_two_to_five_bit_for_bit(n, h, q):
    _, _, _, Q, _, Z1, out = z_case(n, h, q)
    want = rc.scaled(Z1, Q, out["coef_q"], out["resid_mean"], np.ones(h), out["flat"], np.inf)
    assert out["Z"].dtype == np.float32 and np.array_equal(out["Z"], want)
    assert not out["flat"].any() and out["coef_q"].shape == (q, h)
    c64, _ = rc.coefficients(Z1, Q)
    bound = 2 * (n + 2) * 2.0 ** -53 * np.outer(np.linalg.norm(Q, axis=0), np.linalg.norm(Z1.astype(np.float64), axis=0))
    assert np.all(np.abs(out["coef_q"] - c64) <= bound)
    _, _, var = rc.moments(rc.residuals(Z1, Q, out["coef_q"]), out["resid_mean"])
    np.testing.assert_allclose(out["resid_var"], var, rtol=RTOL, atol=0.0)


@pytest.mark.parametrize("n,h,q", Z_SHAPES)
def test_columns_are_orthogonal_to_the_design(n, h, q):
    _, _, _, Q, _, _, out = z_case(n, h, q)
    Z = out["Z"].astype(np.float64)
    assert np.all(np.abs(Z.T @ Q) <= 2 * 2.0 ** -24 * np.linalg.norm(Z, axis=0)[:, None])


# ---- sparse equals dense, run equals run ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,h,q", [(257, 65, 2), (1027, 129, 9), (255, 1, 1)])
def test_sparse_equals_dense_and_run_equals_run(n, h, q):
    X, lu, b0, b1, alpha = residual_inputs(n, G_Z, seed=9)
    X, A = rc.csr_with_stored_zeros_and_empty_row(X, np.random.default_rng(n))
    rng = np.random.default_rng(h)
    genes = rng.permutation(G_Z)[:h]
    Q = rc.intercept_basis(n) if q == 1 else preprocess.design_basis(rc.covariates(rng, X, q - 1))[0]
    V = rng.normal(size=(h, min(h, 5))).astype(np.float32)
    par = (b0[genes], b1[genes], alpha[genes])
    cells = np.sort(rng.permutation(n)[:min(n, 200)])
    cells = cells[cells != 3]                                    # (the emptied row would be a constant zero count: legal, but dull)
    results = []
    with ExpressionMatrix(X) as d, ExpressionMatrix(A) as s:
        assert s.sparse and not d.sparse
        for m in (d, s, d, s):
            out = {"log1p": m.gene_log1p_sum()}
            fit = m.nb_fit(cells, genes, lu[cells])
            out.update({key: fit[key] for key in FIT_KEYS})
            out["moment_mean"], out["moment_var"] = m.sct_residual_moments(genes, *par, lu)
            out["Z1"] = m.select_pearson(genes, *par, lu, center=False).fetch_scaled()
            m.select_pearson(genes, *par, lu, Q=Q)
            out.update({"Z": m.fetch_scaled(), "coef_q": m.coef_q, "resid_mean": m.resid_mean, "resid_var": m.resid_var,
                        "flat": m.flat, "gram": m.gram(), "project": m.project(V)})
            results.append(out)
    for other in results[1:]:
        for key, want in results[0].items():
            assert other[key].dtype == want.dtype and np.array_equal(other[key], want, equal_nan=True), key
    assert results[0]["Z"].any() and not np.isnan(results[0]["gram"]).any() and np.isfinite(results[0]["b1"]).all()


# ---- error codes ----------------------------------------------------------------------------------------------------------------

def code_of(fn, *args, **kw):
    with pytest.raises(_lib.MiSaError) as ei:
        fn(*args, **kw)
    return ei.value.code


def test_errors():
    import ctypes as C
    X, lu, b0, b1, alpha = residual_inputs(12, 6)
    cells, genes, one = np.arange(12), np.arange(3), np.ones(3)
    f64p = C.POINTER(C.c_double)
    with ExpressionMatrix(X) as m:
        lib, h = m._lib, m._handle()
        # NULL pointers, straight at the C entries
        assert lib.mi_prep_gene_log1p_sum(h, None, None) == EINVAL and lib.mi_prep_gene_log1p_sum(None, None, None) == EINVAL
        assert lib.mi_prep_nb_fit(h, None, 12, None, 3, None, None, None, None, None, None, None, None, None, None, None) == EINVAL
        assert lib.mi_prep_sct_residual_moments(h, None, 3, None, None, None, None, 3.0, None, None, None) == EINVAL
        assert lib.mi_prep_sct_select(h, None, 3, None, None, None, None, 3.0, None, 1, None, None, None, None, None) == EINVAL
        # the fit
        assert code_of(m.nb_fit, cells[:2], genes, lu[:2]) == EINVAL                         # fewer than 3 cells
        assert code_of(m.nb_fit, cells, genes[:0], lu) == EINVAL
        assert code_of(m.nb_fit, [0, 1, 12], genes, lu[:3]) == EINVAL                        # out of range
        assert code_of(m.nb_fit, [0, 1, 1], genes, lu[:3]) == EINVAL                         # repeated
        assert code_of(m.nb_fit, cells, [0, 6], lu) == EINVAL
        assert code_of(m.nb_fit, cells, [2, 2], lu) == EINVAL
        assert code_of(m.nb_fit, cells, genes, np.full(12, 3.0)) == EINVAL                   # no spread in the covariate
        with pytest.raises(ValueError):
            m.nb_fit(cells, genes, np.where(cells == 4, -np.inf, lu))                       # a cell without counts
        bad = lu.copy()
        bad[4] = np.nan
        i32 = np.zeros(8193, dtype=np.int32)
        f64 = np.zeros(8193)
        ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        outs = [ptr(f64, C.c_double)] * 6 + [ptr(i32, C.c_int32), ptr(i32, C.c_uint8), ptr(i32, C.c_uint8)]
        assert lib.mi_prep_nb_fit(h, ptr(i32, C.c_int32), 12, ptr(i32, C.c_int32), 3, bad.ctypes.data_as(f64p), *outs,
                                  None) == EINVAL                                            # (repeated cells, in fact)
        assert lib.mi_prep_nb_fit(h, ptr(i32, C.c_int32), 8193, ptr(i32, C.c_int32), 3, ptr(f64, C.c_double), *outs,
                                  None) == EUNSUPPORTED                                      # more than 8192 fit cells
        assert lib.mi_prep_nb_fit(h, ptr(i32, C.c_int32), 12, ptr(i32, C.c_int32), 4097, ptr(f64, C.c_double), *outs,
                                  None) == EUNSUPPORTED                                      # more than 4096 fit genes
        c12 = np.arange(12, dtype=np.int32)
        assert lib.mi_prep_nb_fit(h, ptr(c12, C.c_int32), 12, ptr(c12, C.c_int32), 3, bad.ctypes.data_as(f64p), *outs,
                                  None) == EINVAL                                            # a non-finite log_umi
        # the residual moments
        p3 = (b0[:3], b1[:3], alpha[:3])
        assert code_of(m.sct_residual_moments, [0, 1, 6], *p3, lu) == EINVAL
        assert code_of(m.sct_residual_moments, [0, 1, 1], *p3, lu) == EINVAL
        assert code_of(m.sct_residual_moments, genes[:0], b0[:0], b1[:0], alpha[:0], lu) == EINVAL
        assert code_of(m.sct_residual_moments, genes, b0[:3], b1[:3], -one, lu) == EINVAL    # a negative alpha
        assert code_of(m.sct_residual_moments, genes, b0[:3], one * np.inf, alpha[:3], lu) == EINVAL
        assert code_of(m.sct_residual_moments, genes, one * np.nan, b1[:3], alpha[:3], lu) == EINVAL
        assert code_of(m.sct_residual_moments, genes, *p3, lu, 0.0) == EINVAL
        assert code_of(m.sct_residual_moments, genes, *p3, lu, np.nan) == EINVAL
        with pytest.raises(ValueError):
            m.sct_residual_moments(genes, *p3, bad)
        # the selection
        m.select_pearson(genes, *p3, lu)
        assert m.fetch_scaled().shape == (12, 3)
        for args, kw, code in ((([0, 1, 6], *p3, lu), {}, EINVAL), (([0, 1, 1], *p3, lu), {}, EINVAL),
                               ((genes, b0[:3], b1[:3], -one, lu), {}, EINVAL), ((genes, *p3, lu), {"clip": 0.0}, EINVAL),
                               ((genes, *p3, lu), {"clip": np.nan}, EINVAL),
                               ((genes, *p3, lu), {"Q": np.full((12, 1), np.inf)}, EINVAL),
                               ((genes, *p3, lu), {"Q": np.ones((12, 10))}, EUNSUPPORTED),
                               ((genes[:0], b0[:0], b1[:0], alpha[:0], lu), {}, EINVAL)):
            assert code_of(m.select_pearson, *args, **kw) == code
            assert code_of(m.fetch_scaled) == ESTATE and code_of(m.gram) == ESTATE          # nothing is left selected
            m.select_pearson(genes, *p3, lu)
        big = np.zeros(4097)
        assert code_of(m.select_pearson, np.zeros(4097, dtype=np.int32), big, big, big, lu) == EUNSUPPORTED
        assert code_of(m.fetch_scaled) == ESTATE
        with pytest.raises(ValueError):
            m.select_pearson(genes, *p3, lu, Q=np.ones((12, 1)), center=False)
    Xz = X.copy()
    Xz[5] = 0.0
    with pytest.raises(ValueError, match="no counts"):
        preprocess.sctransform(Xz)


# ---- the driver -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reference_chain(regress):
    X, groups, _ = sc.planted_counts()
    cov = sc.planted_covariate() if regress else None
    return X, groups, cov, sr.sctransform(X, variable_features_n=200, npcs=10, vars_to_regress=cov)


@pytest.mark.parametrize("kind", ["dense", "csr"])
@pytest.mark.parametrize("regress", [False, True])
def test_driver_on_planted_groups(regress, kind):
    X, groups, cov, want = reference_chain(regress)
    n = X.shape[0]
    r = preprocess.sctransform(sp.csr_matrix(X) if kind == "csr" else X, variable_features_n=200, npcs=10, vars_to_regress=cov)
    assert r.coords.shape == (n, 10) and r.coords.dtype == np.float32 and len(r.genes) == 200
    assert set(r.genes.tolist()) == set(want["genes"].tolist())
    assert np.array_equal(r.model.genes, want["genes1"]) and r.model.converged.all()
    assert np.array_equal(r.gene_attr.detected, (X != 0).sum(axis=0))
    np.testing.assert_allclose(r.gene_attr.log_gmean, sr.gene_attributes(X)[1], rtol=1e-9)
    np.testing.assert_allclose(r.gene_attr.residual_variance[want["passing"]], want["residual_variance"], rtol=1e-6)
    for key in ("nb_fit_ms", "sct_moments_ms", "sct_select_ms", "gram_ms", "project_ms", "sct_regularize_s"):
        assert r.timing[key] >= 0.0, key
    assert ("regression" in r) == regress
    # the coordinates: the restatement's scaled matrix (its columns in the device's order) on the device's loadings, within
    # the projection's bound plus what the entries of Z that differ by a float32 rounding carry
    order = np.array([np.flatnonzero(want["genes"] == j)[0] for j in r.genes])
    Zw = want["Z"][:, order]
    V32 = r.loadings.astype(np.float32)
    with ExpressionMatrix(X) as m:
        a = r.gene_attr
        Q = None if cov is None else preprocess.design_basis(cov, n=n)[0]
        Z = m.select_pearson(r.genes, a.b0[r.genes], a.b1[r.genes], a.alpha[r.genes], r.log_umi, Q=Q).fetch_scaled()
    dZ = np.abs(Z - Zw)
    assert np.all(dZ <= 2.0 ** -22 * np.maximum(np.abs(Zw), 1.0))
    bound = ref.project_bound(Zw, V32) + dZ @ np.abs(V32.astype(np.float64))
    assert np.all(np.abs(r.coords - Zw @ V32.astype(np.float64)) <= bound)
    # ... and, after aligning signs, the restatement's own leading coordinates: the two group axes, whose eigenvalues stand
    # forty-fold above the rest (the axes inside that pair turn freely when the pair is close, so the pair is compared as a plane)
    P, Pw = r.coords[:, :2].astype(np.float64), want["coords"][:, :2]
    rot, _, _, _ = np.linalg.lstsq(P, Pw, rcond=None)
    assert np.abs(P @ rot - Pw).max() <= 1e-3 * np.abs(Pw).max()
    assert np.abs(rot.T @ rot - np.eye(2)).max() <= 1e-3
    g = snn.build_snn(r.coords[:, :2], k=10)
    rows = np.repeat(np.arange(n), np.diff(g.rowptr))
    assert len(g.col) > 0 and np.array_equal(groups[rows], groups[g.col])      # no edge joins two planted groups
