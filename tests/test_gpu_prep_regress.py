"""Cell QC (``mi_prep_cell_qc``) and the regression of covariates (``mi_prep_select_regressed``, ``vars_to_regress``) on the
device, against the numpy restatement of tests/prep_regress_cases.py.

Shapes are the kernels' edges: the row slice of 256 (n = 2, 255, 256, 257, 1027: one, two and five slices, the four row
lanes), the 64-column workgroup and the 128-column padding of Z (h = 1, 63, 64, 65, 128, 129), the design's width (q = 1, 2,
9 = MI_PREP_MAX_DESIGN_COLS); each n with h = 65 and q = 2, each h and each q with n = 257.

Every bound is derived, none measured:
  coefficients  |c - Q^T Y64|_kj <= 2 (n + 2) 2^-53 |q_k| |y_j|: the standard summation bound of an n-term dot product, once
                for the device and once for numpy;
  mean          |mean - ref| <= 2 (n - 1) 2^-53 sum |r_i| / n, likewise; the variance within the project's fp64 RTOL, about
                the device's own mean (the second pass uses it);
  Z             bit for bit the numpy fp64 expression built from the device's c, mean, var and flat;
  orthogonality with clip = 1e30, |sum_i z_ij Q_ik| <= 2 * 2^-24 sqrt(n - 1): each z carries one f32 rounding,
                |z_j| = sqrt(n - 1), |q_k| = 1, a margin of 2;
  intercept     with q = 1, |z - ref| <= 2^-24 |ref| + 1e-12 (|y| + |mean|) / sd against ScaleData's fp64 expression of the
                device's gene statistics;
  end to end    |corr(coords_k, u)| <= (h + 3) 2^-24 sqrt(h / lambda_k): coords_k = Z v_k with every column of the exact
                scaled residuals orthogonal to u and to 1, so what remains is the f32 rounding of Z (2^-24 |z_i| per cell)
                and ``project_bound`` ((h + 2) 2^-24 |z_i|), |z_i| <= sqrt(h) max |z|, against |coords_k| = sqrt((n - 1)
                lambda_k)."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import prep_reference as ref
import prep_regress_cases as cases
from scrna_seq_qannealing_clustering_amd import _lib, preprocess, snn
from scrna_seq_qannealing_clustering_amd.preprocess import ExpressionMatrix

pytestmark = pytest.mark.gpu

RTOL = 1e-9                                   # the project's fp64 tolerance (tests/test_gpu_prep.py)
EINVAL, EUNSUPPORTED, ESTATE = -1, -5, -6
G = 150
SHAPES = ([(n, 65, 2) for n in (2, 255, 256, 257, 1027)] + [(257, h, 2) for h in (1, 63, 64, 128, 129)] +
          [(257, 65, q) for q in (1, 9)])


def inputs(n, h, q):
    """-> counts, the chosen genes (shuffled), Q"""
    rng = np.random.default_rng(100000 * q + 1000 * n + h)
    X = ref.sparse_counts(rng, n, G)
    genes = rng.permutation(G)[:h]
    Q = cases.intercept_basis(n) if q == 1 else preprocess.design_basis(cases.covariates(rng, X, q - 1))[0]
    assert Q.shape == (n, q)
    return X, genes, Q


def outputs(m, genes, Q, clip):
    m.select_regressed(genes, Q, clip)
    return {"Z": m.fetch_scaled(), "coef_q": m.coef_q, "resid_mean": m.resid_mean, "resid_var": m.resid_var, "flat": m.flat}


@functools.lru_cache(maxsize=None)
def device_case(n, h, q):
    """one dense handle per shape: the device's Y, and every output at clip 10 and at clip 1e30 (computed once, never changed)"""
    X, genes, Q = inputs(n, h, q)
    with ExpressionMatrix(X) as m:
        Y = m.normalize().fetch_normalized()
        stats = m.gene_stats("normalized")
        clipped, open_ = outputs(m, genes, Q, 10.0), outputs(m, genes, Q, 1e30)
        assert m.timing["regress_ms"] >= 0.0
    return X, genes, Q, Y[:, genes], stats, clipped, open_


# ---- 1. - 3., 5.: coefficients, moments, Z bit for bit, orthogonality -------------------------------------------------------

@pytest.mark.parametrize("n,h,q", SHAPES)
def test_coefficients(n, h, q):
    _, _, Q, Yg, _, out, _ = device_case(n, h, q)
    c64, _ = cases.coefficients(Yg, Q)
    assert out["coef_q"].shape == (q, h) and out["coef_q"].dtype == np.float64
    bound = 2 * (n + 2) * 2.0 ** -53 * np.outer(np.linalg.norm(Q, axis=0), np.linalg.norm(Yg.astype(np.float64), axis=0))
    assert np.abs(c64).max() > 0.1
    assert np.all(np.abs(out["coef_q"] - c64) <= bound)


@pytest.mark.parametrize("n,h,q", SHAPES)
def test_moments(n, h, q):
    _, _, Q, Yg, _, out, _ = device_case(n, h, q)
    r = cases.residuals(Yg, Q, out["coef_q"])
    mean, _, _ = cases.moments(r)
    assert np.all(np.abs(out["resid_mean"] - mean) <= 2 * (n - 1) * 2.0 ** -53 * np.abs(r).sum(axis=0) / n)
    _, _, var = cases.moments(r, out["resid_mean"])
    np.testing.assert_allclose(out["resid_var"], var, rtol=RTOL, atol=0.0)
    assert out["flat"].dtype == np.bool_ and out["flat"].shape == (h,)
    if n > q + 1:
        assert not out["flat"].any() and (out["resid_var"] > 0).all()


@pytest.mark.parametrize("n,h,q", SHAPES)
def test_scaled_residuals_bit_for_bit(n, h, q):
    _, _, Q, Yg, _, clipped, open_ = device_case(n, h, q)
    for out, clip in ((clipped, 10.0), (open_, 1e30)):
        Z = out["Z"]
        assert Z.shape == (n, h) and Z.dtype == np.float32
        want = cases.scaled(Yg, Q, out["coef_q"], out["resid_mean"], out["resid_var"], out["flat"], clip)
        assert np.array_equal(Z, want)
    for key in ("coef_q", "resid_mean", "resid_var", "flat"):                  # the clip touches the last stage alone
        assert np.array_equal(clipped[key], open_[key]), key
    assert np.array_equal(np.minimum(open_["Z"], np.float32(10.0)), clipped["Z"])
    if n > q + 1:
        assert clipped["Z"].any(axis=0).all()


@pytest.mark.parametrize("n,h,q", SHAPES)
def test_unclipped_columns_are_orthogonal_to_the_design(n, h, q):
    _, _, Q, _, _, _, out = device_case(n, h, q)
    dots = out["Z"].astype(np.float64).T @ Q
    assert np.all(np.abs(dots) <= 2 * 2.0 ** -24 * np.sqrt(n - 1))


# ---- 4. flat columns --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["dense", "csr"])
def test_flat_columns(kind):
    """an all-zero gene, a gene constant after normalisation and a gene in the span of the design (the covariate is built from
    its normalised column: y = 2 covariate + 1 up to the rounding of the construction) come out exactly zero with flat = 1;
    a gene with one non-zero cell among 257 does not"""
    X = cases.flat_columns_counts(np.random.default_rng(2))
    names = cases.FLAT_GENES
    genes = np.array([7, names["one_cell"], names["in_span"], 11, names["constant"], names["zero"], names["filler"]])
    with ExpressionMatrix(X) as d:
        Y = d.normalize().fetch_normalized()
    assert len(set(Y[:, names["constant"]].tolist())) == 1 and Y[0, names["constant"]] > 0
    cov = (Y[:, names["in_span"]].astype(np.float64) - 1.0) / 2.0
    Q, R = preprocess.design_basis(cov)
    with ExpressionMatrix(sp.csr_matrix(X) if kind == "csr" else X) as m:
        out = outputs(m.normalize(), genes, Q, 10.0)
    assert out["flat"].tolist() == [False, False, True, False, True, True, False]
    Z = out["Z"]
    assert not Z[:, out["flat"]].any() and Z[:, ~out["flat"]].any(axis=0).all()
    assert np.array_equal(Z, cases.scaled(Y[:, genes], Q, out["coef_q"], out["resid_mean"], out["resid_var"], out["flat"], 10.0))
    betas = preprocess.regression_betas(R, out["coef_q"])
    np.testing.assert_allclose(betas[:, 2], [1.0, 2.0], rtol=1e-12)             # the model of the gene in the span
    np.testing.assert_allclose(betas[:, 5], [0.0, 0.0], atol=0.0)
    assert np.argmax(Z[:, 1]) == 5 and Z[5, 1] > 0                              # the one cell with a count stands out


# ---- 6. intercept only is ScaleData ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,h", [(257, 65), (1027, 129)])
def test_intercept_only_is_scale_data(n, h):
    X, genes, Q = inputs(n, h, 1)
    with ExpressionMatrix(X) as m:
        Y = m.normalize().fetch_normalized()[:, genes].astype(np.float64)
        mean, var, _ = m.gene_stats("normalized")
        Z = m.select_regressed(genes, Q, 10.0).fetch_scaled()
    mu, sd = mean[genes], np.sqrt(var[genes])
    assert (sd > 0).all()
    want = np.minimum((Y - mu) / sd, 10.0)
    assert np.all(np.abs(Z - want) <= 2.0 ** -24 * np.abs(want) + 1e-12 * (np.abs(Y) + np.abs(mu)) / sd)


# ---- 6b. the order of the reductions, bit for bit ---------------------------------------------------------------------------

ORDER_SHAPES = ([(n, 65, 2) for n in (2, 5, 257, 1027)] + [(257, h, 2) for h in (1, 63, 130)] + [(257, 65, q) for q in (1, 9)])


@pytest.mark.parametrize("n,h,q", ORDER_SHAPES)
def test_regression_order_bit_for_bit(n, h, q):
    """coef_q, resid_mean and resid_var of a dense handle are the bits of the documented order restated in numpy on the
    gathered columns of the device's Y (prep_reference.ordered_regression); from two slices on, plain ascending sums give
    other coefficients, means and variances"""
    rng = np.random.default_rng(9000 * q + 70 * n + h)
    X = ref.fractional_counts(rng, n, G)
    genes = rng.permutation(G - 2)[:h]
    if h >= 3:
        genes[-2:] = [G - 1, G - 2]                              # (the all-zero and the constant column)
    Q = cases.intercept_basis(n) if q == 1 else preprocess.design_basis(cases.covariates(rng, X, q - 1))[0]
    with ExpressionMatrix(X) as m:
        Yg = m.normalize().fetch_normalized()[:, genes]
        m.select_regressed(genes, Q, 10.0)
        got = (m.coef_q, m.resid_mean, m.resid_var)
    want = ref.ordered_regression(Yg, Q)
    if n >= 257:
        for plain, ordered in zip(ref.ordered_regression(Yg, Q, ref.plain_column_sum), want):
            assert (plain != ordered).any()                      # (coefficients, means and variances alike)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


# ---- 7. sparse equals dense, run equals run -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n,h,q", [(257, 65, 2), (1027, 65, 2), (257, 129, 9), (255, 1, 1)])
def test_sparse_equals_dense_and_run_equals_run(n, h, q):
    X, genes, Q = inputs(n, h, q)
    X, A = cases.csr_with_stored_zeros_and_empty_row(X, np.random.default_rng(n))
    V = np.random.default_rng(h).normal(size=(h, min(h, 5))).astype(np.float32)
    with ExpressionMatrix(X) as d, ExpressionMatrix(A) as s:
        assert s.sparse and not d.sparse
        Y = d.normalize().fetch_normalized()
        s.normalize()
        results = []
        for m in (d, s, d, s):
            out = outputs(m, genes, Q, 10.0)
            out["gram"], out["project"] = m.gram(), m.project(V)
            results.append(out)
        # a plain select afterwards is what it was: the regression leaves nothing behind in the handle
        mean, var, _ = d.gene_stats("normalized")
        plain = [m.select(genes, mean[genes], np.sqrt(var[genes]), 10.0).fetch_scaled() for m in (d, s)]
    for other in results[1:]:
        for key, want in results[0].items():
            assert other[key].dtype == want.dtype and np.array_equal(other[key], want), key
    assert results[0]["Z"].any() and not np.isnan(results[0]["gram"]).any()
    assert np.array_equal(plain[0], plain[1])
    assert np.array_equal(plain[0], ref.scaled(Y, genes, mean[genes], np.sqrt(var[genes]), 10.0))


# ---- 8. cell QC -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("n", [2, 5, 257])
def test_cell_qc(n, g):
    rng = np.random.default_rng(1000 * n + g)
    X = ref.sparse_counts(rng, n, g, rate=0.6)
    X[0, 0] = 3.0
    X[1] = 0.0                                                   # a cell without counts
    masks = {"none": None, "empty": np.zeros(g, dtype=bool), "full": np.ones(g, dtype=bool), "random": rng.random(g) < 0.3,
             "gene64": np.arange(g) == 64}                       # (gene 64 alone: lane 0's second column; empty for g <= 64)
    X, A = cases.csr_with_stored_zeros_and_empty_row(X, rng) if n > 3 else (X, sp.csr_matrix(X))
    X64 = X.astype(np.float64)
    tot = X64.sum(axis=1)
    assert tot[1] == 0.0 and tot.any()
    with ExpressionMatrix(X) as d, ExpressionMatrix(A) as s:
        for name, mask in masks.items():
            for m in (d, s):
                n_count, n_feature, subset = m.cell_qc(mask)
                assert n_count.dtype == np.float64 and n_feature.dtype == np.int32 and m.timing["qc_ms"] >= 0.0
                # integer counts: every sum is exact in any order
                assert np.array_equal(n_count, X64.sum(axis=1)), name
                assert np.array_equal(n_feature, (X != 0).sum(axis=1)), name
                if mask is None:
                    assert subset is None
                else:
                    assert subset.dtype == np.float64 and np.array_equal(subset, X64[:, mask].sum(axis=1)), name
            qd, qs = preprocess.cell_qc(d, mask=mask), preprocess.cell_qc(s, mask=mask)
            if mask is None:
                assert qd.percent is None and qs.percent is None
            else:
                assert np.array_equal(qd.percent, qs.percent) and qd.percent[1] == 0.0
                assert np.array_equal(qd.percent, np.where(tot > 0, 100.0 * X64[:, mask].sum(axis=1) / np.where(tot > 0, tot, 1.0), 0.0))
                if name == "full":
                    assert np.array_equal(qd.percent, np.where(tot > 0, 100.0, 0.0))
        # n_count is the total the normaliser divides by: log1p(x * 1e4 / n_count) is the device's Y within one ulp
        n_count, _, _ = d.cell_qc()
        Y = d.normalize().fetch_normalized()
        safe = np.where(n_count > 0, n_count, 1.0)[:, None]
        host = np.where(n_count[:, None] > 0, np.log1p(X64 * 1e4 / safe), 0.0).astype(np.float32)
        assert (np.abs(Y.view(np.int32).astype(np.int64) - host.view(np.int32)) <= 1).all()
        assert np.array_equal(s.normalize().fetch_normalized().toarray(), Y)


def test_cell_qc_by_gene_names_and_filter():
    rng = np.random.default_rng(9)
    X = ref.sparse_counts(rng, 40, 30, rate=0.6)
    names = ["MT-%d" % j if j % 7 == 0 else ("mt-%d" % j if j % 7 == 1 else "G%d" % j) for j in range(30)]
    mask = np.arange(30) % 7 == 0
    qc = preprocess.cell_qc(sp.csc_matrix(X), names)
    want = preprocess.cell_qc(X, mask=mask)
    for key in ("n_count", "n_feature", "percent"):
        assert np.array_equal(qc[key], want[key]), key
    assert np.array_equal(qc.percent, 100.0 * X[:, mask].astype(np.float64).sum(axis=1) / X.astype(np.float64).sum(axis=1))
    keep = preprocess.qc_filter(qc, min_features=10, max_features=25, max_percent=20.0)
    assert np.array_equal(keep, (qc.n_feature > 10) & (qc.n_feature < 25) & (qc.percent < 20.0)) and 0 < keep.sum() < 40
    with pytest.raises(ValueError):
        preprocess.cell_qc(X, names[:-1])
    with pytest.raises(ValueError):
        preprocess.cell_qc(X, mask=np.ones(30, dtype=np.uint8))                  # not boolean


# ---- 9. error codes -------------------------------------------------------------------------------------------------------------

def test_errors():
    lib = _lib.load()
    f64p, i32p, u8p, f32p = (C.POINTER(t) for t in (C.c_double, C.c_int32, C.c_uint8, C.c_float))
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
    X = ref.sparse_counts(np.random.default_rng(8), 10, 6)
    Q = preprocess.design_basis(np.arange(10.0))[0]
    genes = np.array([0, 1, 2], dtype=np.int32)
    buf = np.zeros(60, dtype=np.float32)
    nc, nf, sub = np.zeros(10), np.zeros(10, dtype=np.int32), np.zeros(10)

    def qc(m, mask, n_count, n_feature, subset):
        return lib.mi_prep_cell_qc(m, ptr(mask, u8p), ptr(n_count, f64p), ptr(n_feature, i32p), ptr(subset, f64p), None)

    def regressed(m, genes, h, Q, q, clip):
        return lib.mi_prep_select_regressed(m, ptr(genes, i32p), h, ptr(Q, f64p), q, clip, None, None, None, None, None)

    def changed(a, at, value):
        b = a.copy()
        b[at] = value
        return b
    for M in (X, sp.csr_matrix(X)):
        with ExpressionMatrix(M) as m:
            hd = m._handle()
            mask = np.array([1, 0, 0, 1, 0, 0], dtype=np.uint8)
            assert qc(None, mask, nc, nf, sub) == EINVAL
            assert qc(hd, changed(mask, 5, 2), nc, nf, sub) == EINVAL
            assert b"gene_mask[5]" in lib.mi_last_error()
            assert qc(hd, None, nc, nf, sub) == EINVAL                           # subset_count without a mask
            assert qc(hd, None, nc, nf, None) == 0 and qc(hd, mask, None, None, None) == 0
            assert qc(hd, mask, nc, nf, sub) == 0 and np.array_equal(sub, X[:, [0, 3]].sum(axis=1))
            assert regressed(hd, genes, 3, Q, 2, 10.0) == ESTATE                 # before normalize
            m.normalize()
            fetch = lambda: lib.mi_prep_fetch_scaled(hd, buf.ctypes.data_as(f32p))
            for args, code in (((None, genes, 3, Q, 2, 10.0), EINVAL),
                               ((hd, None, 3, Q, 2, 10.0), EINVAL),
                               ((hd, genes, 3, None, 2, 10.0), EINVAL),
                               ((hd, genes, 0, Q, 2, 10.0), EINVAL),
                               ((hd, genes, 3, Q, 0, 10.0), EINVAL),
                               ((hd, changed(genes, 1, 6), 3, Q, 2, 10.0), EINVAL),
                               ((hd, changed(genes, 1, -1), 3, Q, 2, 10.0), EINVAL),
                               ((hd, changed(genes, 2, 0), 3, Q, 2, 10.0), EINVAL),       # chosen twice
                               ((hd, genes, 3, changed(Q, (9, 1), np.nan), 2, 10.0), EINVAL),
                               ((hd, genes, 3, changed(Q, (0, 0), np.inf), 2, 10.0), EINVAL),
                               ((hd, genes, 3, Q, 2, np.nan), EINVAL),
                               ((hd, genes, 3, Q, 2, 0.0), EINVAL),
                               ((hd, genes, 3, Q, 2, -1.0), EINVAL),
                               ((hd, np.zeros(4097, dtype=np.int32), 4097, Q, 2, 10.0), EUNSUPPORTED),
                               ((hd, genes, 3, np.zeros((10, 10)), 10, 10.0), EUNSUPPORTED)):
                assert regressed(hd, genes, 3, Q, 2, 10.0) == 0 and fetch() == 0
                assert regressed(*args) == code, args[2:]
                assert args[0] is None or fetch() == ESTATE                      # a failed call leaves nothing selected
            with pytest.raises(_lib.MiSaError) as ei:
                m.select_regressed(genes, Q, 10.0).select_regressed([0, 1, 1], Q, 10.0)
            assert ei.value.code == EINVAL and m.h == 0
            with pytest.raises(_lib.MiSaError) as ei:
                m.gram()
            assert ei.value.code == ESTATE
            with pytest.raises(ValueError):
                m.select_regressed(genes, Q[:9], 10.0)                           # one row of Q per cell
            with pytest.raises(ValueError):
                preprocess.scale_data(m, genes, vars_to_regress=np.ones(10))     # a constant covariate
            with pytest.raises(ValueError):
                preprocess.pca(m, genes, npcs=2, vars_to_regress=np.arange(9.0))
            Z = preprocess.scale_data(m, genes, vars_to_regress=np.arange(10.0))   # the handle survives all of it
            assert Z.shape == (10, 3) and m.regression.betas.shape == (2, 3) and np.array_equal(m.regression.flat, m.flat)
            assert preprocess.scale_data(m, genes).shape == (10, 3) and m.regression is None


# ---- 10. end to end -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1, 2])
def test_nuisance_factor_end_to_end(seed):
    X, groups, u = cases.planted_counts_with_nuisance(seed)
    n, h = X.shape
    genes = np.arange(h)
    with ExpressionMatrix(sp.csr_matrix(X) if seed == 1 else X) as m:
        m.normalize()
        # (a) unclipped, no PC remembers u
        r = preprocess.pca(m, genes, npcs=ref.PLANTED_PCS, max_value=1e30, vars_to_regress=u)
        assert not r.regression.flat.any() and r.regression.betas.shape == (2, h) and r.timing["regress_ms"] >= 0.0
        corr = cases.max_abs_corr(r.coords.astype(np.float64), u)
        bound = (h + 3) * 2.0 ** -24 * np.sqrt(h / r.eigenvalues)
        print("seed %d: |corr| %s bound %s" % (seed, corr, bound))
        assert np.all(corr <= bound)
        # the nuisance genes rise with u; the others fall, through the cell totals they are divided by
        assert np.median(r.regression.betas[1, 160:]) > 0 > np.median(r.regression.betas[1, :160])
        # (b) with the default clip the first three PCs separate the planted groups
        r = preprocess.pca(m, genes, npcs=ref.PLANTED_PCS, vars_to_regress=u)
        g = snn.build_snn(r.coords[:, :3], k=10)
        rows = np.repeat(np.arange(n), np.diff(g.rowptr))
        assert len(g.col) > 0 and np.array_equal(groups[rows], groups[g.col])    # no edge joins two planted groups
        # (c) the control: without the regression one of them follows u
        plain = preprocess.pca(m, genes, npcs=ref.PLANTED_PCS)
        assert "regression" not in plain
        assert cases.max_abs_corr(plain.coords[:, :3].astype(np.float64), u).max() > 0.5


def test_embed_with_vars_to_regress():
    """the intended use: QC columns, the filter, then embed with percent regressed out; sparse in, the same bits"""
    X, _, u = cases.planted_counts_with_nuisance(0)
    names = ["MT-%d" % j if j >= 160 else "G%d" % j for j in range(X.shape[1])]
    qc = preprocess.cell_qc(X, names)
    keep = preprocess.qc_filter(qc, min_features=int(np.median(qc.n_feature)), max_features=None, max_percent=None)
    assert 100 < keep.sum() <= len(keep) // 2
    a = preprocess.embed(X[keep], nfeatures=ref.PLANTED_FEATURES, npcs=5, vars_to_regress=qc.percent[keep])
    b = preprocess.embed(sp.csr_matrix(X[keep]), nfeatures=ref.PLANTED_FEATURES, npcs=5, vars_to_regress=qc.percent[keep])
    assert a.coords.shape == (keep.sum(), 5) and np.array_equal(a.coords, b.coords) and np.array_equal(a.genes, b.genes)
    for key in ("betas", "resid_mean", "resid_var", "flat"):
        assert np.array_equal(a.regression[key], b.regression[key]), key
    assert a.regression.betas.shape == (2, ref.PLANTED_FEATURES)
    plain = preprocess.embed(X[keep], nfeatures=ref.PLANTED_FEATURES, npcs=5)
    assert "regression" not in plain and np.array_equal(plain.genes, a.genes) and not np.array_equal(plain.coords, a.coords)
