"""The preprocessing kernels (csrc/prep_kernels.hip, include/mi_prep.h) against the numpy fp64 reference of
tests/prep_reference.py: the wavefront, row-slice and tile edges of the elementwise and reduction passes; special rows and
columns (an all-zero gene, a constant gene, one huge count that makes both clips bite, a cell without counts, n = 2); the
scaled matrix bit for bit against the float32 numpy expression; the Gram and projection products on the f32-input MFMA
within bounds derived from the f32 chain length (never measured), exact symmetry and run-to-run identity; ``pca``
through Weyl's inequality (no eigenvector is compared component-wise: the bulk is nearly degenerate); the whole chain on
the planted matrix into ``build_snn`` / ``connected_components`` / ``find_all_markers``; and the error codes.

Each chunk of GRAM_CHUNK = C cells is one fmaf chain of at most C terms per entry of G, so
|G - G64|_ab <= (C + 2) 2^-24 sqrt(G64_aa G64_bb), with G64 the fp64 product of the same float32 Z (standard summation
bound + Cauchy-Schwarz); likewise |out - Z64 V64|_ic <= (h + 2) 2^-24 |z_i| |v_c| for the projection."""
import numpy as np
import pytest
import scipy.sparse as sp

import prep_reference as ref
from scrna_seq_qannealing_clustering_amd import _lib, metrics, preprocess, snn
from scrna_seq_qannealing_clustering_amd.preprocess import ExpressionMatrix

pytestmark = pytest.mark.gpu

RTOL = 1e-9                                   # the project's fp64 tolerance (tests/test_gpu_markers.py)
C = preprocess.GRAM_CHUNK
EINVAL, EUNSUPPORTED, ESTATE = -1, -5, -6


def ulps(a, b):
    """distance in float32 steps between two arrays of non-negative floats"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert (a >= 0).all() and (b >= 0).all()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def close(got, want):
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0.0)


def check_passes(X):
    """normalize, gene_stats on both matrices and clipped_variance of one matrix against the reference -> the device's Y"""
    n = X.shape[0]
    with ExpressionMatrix(X) as m:
        Y = m.normalize(1e4).fetch_normalized()
        mean, var, nnz = m.gene_stats("counts")
        ymean, yvar, ynnz = m.gene_stats("normalized")
        sd = np.sqrt(var)
        vs = m.clipped_variance(mean, sd, np.sqrt(n))
        assert all(v >= 0.0 for v in m.timing.values())
    assert Y.dtype == np.float32 and Y.shape == X.shape
    assert ulps(Y, ref.normalize(X, 1e4)).max() <= 1
    rmean, rvar, rnnz = ref.gene_stats(X)
    close(mean, rmean)
    close(var, rvar)
    assert np.array_equal(nnz, rnnz)
    rmean, rvar, rnnz = ref.gene_stats(Y)                        # (of the device's Y: its last bit may differ from numpy's)
    close(ymean, rmean)
    close(yvar, rvar)
    assert np.array_equal(ynnz, rnnz)
    close(vs, ref.clipped_variance(X, mean, sd, np.sqrt(n)))
    return Y


# ---- 1. edges of the elementwise and reduction passes ---------------------------------------------------------------------

@pytest.mark.parametrize("g", [1, 63, 65, 130])
@pytest.mark.parametrize("n", [2, 63, 64, 65, 257])
def test_edges(n, g):
    rng = np.random.default_rng(1000 * n + g)
    check_passes(ref.sparse_counts(rng, n, g))


# ---- 1b. the order of the reductions, bit for bit ---------------------------------------------------------------------------
# n: lanes without a row (2), a lane with two rows (5), a second slice of one row (257), a last slice that fills three lanes
# (1027); g: a partial workgroup of genes (1, 63), two and three workgroups (65, 130).

def same_bits(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("g", [1, 63, 65, 130])
@pytest.mark.parametrize("n", [2, 5, 257, 1027])
def test_reduction_order_bit_for_bit(n, g):
    """mean, variance and nnz of both matrices and the clipped variance, on a dense and on a CSR handle, are the bits of the
    documented order restated in numpy (prep_reference.ordered_*); from two slices on, adding the rows in plain ascending
    order gives other bits, so the comparison does pin the order"""
    X = ref.fractional_counts(np.random.default_rng(7000 * n + g), n, g)
    want = ref.ordered_gene_stats(X)
    if n >= 257:
        plain = ref.ordered_gene_stats(X, ref.plain_column_sum)
        assert (plain[0] != want[0]).any() or (plain[1] != want[1]).any()
    Y = None
    for M in (X, sp.csr_matrix(X)):
        with ExpressionMatrix(M) as m:
            m.normalize(1e4)
            if Y is None:
                Y = m.fetch_normalized()                         # (the device's: log1p is not restated)
            got, ygot = m.gene_stats("counts"), m.gene_stats("normalized")
            sd = np.sqrt(got[1])
            vs = m.clipped_variance(got[0], sd, np.sqrt(n))
        same_bits(got, want)
        same_bits(ygot, ref.ordered_gene_stats(Y))
        same_bits([vs], [ref.ordered_clipped_variance(X, got[0], sd, np.sqrt(n))])


# ---- 2. special rows and columns ------------------------------------------------------------------------------------------

def test_special_columns():
    rng = np.random.default_rng(2)
    n = 300
    X = ref.sparse_counts(rng, n, 6)
    X[:, 0] = 0.0                                                # an all-zero gene
    X[:, 1] = 3.0                                                # a constant non-zero gene
    X[:, 2] = 0.0
    X[17, 2] = 1e6                                               # one huge count
    Y = check_passes(X)
    with ExpressionMatrix(X) as m:
        m.normalize()
        mean, var, nnz = m.gene_stats("counts")
        assert mean[0] == 0.0 and var[0] == 0.0 and nnz[0] == 0
        assert mean[1] == 3.0 and var[1] == 0.0 and nnz[1] == n
        assert nnz[2] == 1
        sd = np.sqrt(var)
        sd[2] = 1.0                                              # an expected sd far below the outlier: the vst clip bites
        vs = m.clipped_variance(mean, sd, np.sqrt(n))
        close(vs, ref.clipped_variance(X, mean, sd, np.sqrt(n)))
        assert vs[0] == 0.0 and vs[1] == 0.0                     # sd == 0 -> 0
        unclipped = ref.clipped_variance(X, mean, sd, np.inf)[2]
        assert vs[2] < unclipped / 100 and abs(vs[2] - (n + (n - 1) * mean[2] ** 2) / (n - 1)) < 1e-6 * vs[2]
        # scaling: sigma == 0 -> zeros (gene 0 by its statistics; gene 3 because the caller says so); max_value bites on gene 2
        ymean, yvar, _ = m.gene_stats("normalized")
        genes = np.array([2, 0, 3, 1])
        sigma = np.sqrt(yvar[genes])
        sigma[2] = 0.0
        assert sigma[1] == 0.0
        Z = m.select(genes, ymean[genes], sigma, 10.0).fetch_scaled()
        assert np.array_equal(Z, ref.scaled(Y, genes, ymean[genes], sigma, 10.0))
        assert not Z[:, 1].any() and not Z[:, 2].any()
        assert Z[17, 0] == 10.0 and (Z[:, 0] < 10.0).sum() == n - 1
        assert Z[:, 3].any()


def test_zero_total_cell_and_two_cells():
    rng = np.random.default_rng(3)
    X = ref.sparse_counts(rng, 70, 9)
    X[[0, 41, 69]] = 0.0
    Y = check_passes(X)
    assert not Y[[0, 41, 69]].any() and Y.any() and np.isfinite(Y).all()
    X2 = np.array([[0.0, 2.0, 5.0], [0.0, 2.0, 0.0]], dtype=np.float32)
    Y2 = check_passes(X2)
    Z = preprocess.scale_data(ExpressionMatrix(X2).normalize(), [2, 1, 0])
    assert np.array_equal(Z, ref.scaled_from_normalized(Y2, [2, 1, 0]))
    assert not Z[:, 2].any()


# ---- 3. select / fetch_scaled ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wide():
    rng = np.random.default_rng(4)
    X = ref.sparse_counts(rng, 65, 130)
    m = ExpressionMatrix(X).normalize()
    yield m, m.fetch_normalized()
    m.close()


@pytest.mark.parametrize("h", [1, 31, 33, 129])
def test_scaled_bit_for_bit(wide, h):
    m, Y = wide
    genes = np.random.default_rng(h).permutation(130)[:h]
    assert h < 3 or np.any(np.diff(genes) < 0)
    mean, var, _ = m.gene_stats("normalized")
    for clip in (10.0, 1.5, np.inf):
        Z = m.select(genes, mean[genes], np.sqrt(var[genes]), clip).fetch_scaled()
        assert Z.shape == (65, h) and Z.dtype == np.float32
        assert np.array_equal(Z, ref.scaled(Y, genes, mean[genes], np.sqrt(var[genes]), clip))
    assert np.array_equal(preprocess.scale_data(m, genes), ref.scaled_from_normalized(Y, genes))


# ---- 4. Gram --------------------------------------------------------------------------------------------------------------

def scaled_handle(n, h, seed):
    rng = np.random.default_rng(seed)
    m = ExpressionMatrix(ref.sparse_counts(rng, n, h, rate=0.5)).normalize()
    preprocess._select_scaled(m, rng.permutation(h), 10.0)
    return m


@pytest.mark.parametrize("n", [2, C - 1, C, C + 1, 2 * C + 3])
@pytest.mark.parametrize("h", [1, 31, 32, 33, 127, 128, 129, 257])
def test_gram(n, h):
    with scaled_handle(n, h, 100 * h + n) as m:
        Z = m.fetch_scaled().astype(np.float64)
        G = m.gram()
        again = m.gram()
    assert n == 2 or Z.any()
    G64 = Z.T @ Z
    assert G.shape == (h, h) and G.dtype == np.float64
    assert np.all(np.abs(G - G64) <= ref.gram_bound(G64, C))
    assert np.array_equal(G, G.T)
    assert np.array_equal(G, again)


def test_gram_hits_diagonal_and_off_diagonal_tiles():
    # h = 257: 3 x 3 blocks of 128, the upper triangle holds 3 diagonal and 3 off-diagonal tiles; every block of G differs
    # from zero and obeys the bound, and the far corner (tile (0, 2), one column wide) is the mirror of (2, 0)
    with scaled_handle(C + 1, 257, 7) as m:
        Z = m.fetch_scaled().astype(np.float64)
        G = m.gram()
    G64 = Z.T @ Z
    for a in range(3):
        for b in range(3):
            blk = (slice(128 * a, 128 * a + 128), slice(128 * b, 128 * b + 128))
            assert np.abs(G64[blk]).max() > 1.0
            assert np.all(np.abs(G[blk] - G64[blk]) <= ref.gram_bound(G64, C)[blk])
    assert np.array_equal(G[:128, 256], G[256, :128])


# ---- 5. projection --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=[33, 257])
def proj(request):
    m = scaled_handle(130, request.param, request.param)
    yield m, m.fetch_scaled()
    m.close()


@pytest.mark.parametrize("p", [1, 2, 50, 64, 65, 128])
def test_project(proj, p):
    m, Z = proj
    h = Z.shape[1]
    V = np.random.default_rng(p).normal(size=(h, p)).astype(np.float32)
    out = m.project(V)
    assert out.shape == (130, p) and out.dtype == np.float32
    want = Z.astype(np.float64) @ V.astype(np.float64)
    assert np.abs(want).max() > 1.0
    assert np.all(np.abs(out - want) <= ref.project_bound(Z, V))
    assert np.array_equal(out, m.project(V))
    # an asymmetric operand: e_c picks column c of Z exactly (a row / column swap in the store would not survive this)
    E = np.zeros((h, p), dtype=np.float32)
    E[np.arange(p) * 3 % h, np.arange(p)] = 1.0
    assert np.array_equal(m.project(E), Z[:, np.arange(p) * 3 % h])


# ---- 6. pca ---------------------------------------------------------------------------------------------------------------

def test_pca():
    X, _ = ref.planted_counts(5)
    n, npcs = X.shape[0], ref.PLANTED_PCS
    with ExpressionMatrix(X) as m:
        m.normalize()
        feats = preprocess.find_variable_features(m, nfeatures=ref.PLANTED_FEATURES)
        r = preprocess.pca(m, feats.genes, npcs=npcs)
        Z = m.fetch_scaled()
    G64 = Z.astype(np.float64).T @ Z.astype(np.float64)
    eps = np.linalg.norm(ref.gram_bound(G64, C)) / (n - 1)       # Frobenius norm >= spectral norm of the Gram error / (n - 1)
    want = np.linalg.eigvalsh(G64 / (n - 1))[::-1]
    assert np.all(np.abs(r.eigenvalues - want[:npcs]) <= eps)    # Weyl
    V = r.loadings
    assert np.linalg.norm(G64 / (n - 1) @ V - V * r.eigenvalues, axis=0).max() <= eps
    assert np.abs(V.T @ V - np.eye(npcs)).max() <= 1e-10
    assert np.all(V[np.argmax(np.abs(V), axis=0), np.arange(npcs)] > 0)
    assert np.allclose(r.stdev, np.sqrt(r.eigenvalues)) and abs(r.total_variance - want.sum()) <= eps * len(want)
    V32 = V.astype(np.float32)
    assert r.coords.shape == (n, npcs)
    assert np.all(np.abs(r.coords - Z.astype(np.float64) @ V32.astype(np.float64)) <= ref.project_bound(Z, V32))
    for key in ("normalize_ms", "gene_stats_counts_ms", "clipped_variance_ms", "select_ms", "gram_ms", "project_ms",
                "eigh_s", "loess_s"):
        assert r.timing[key] >= 0.0, key
    # the device's variable-gene table against the reference's, same loess
    genes, vs = ref.variable_features(X, ref.PLANTED_FEATURES, preprocess.loess_fit)
    close(feats.variance_standardized, vs)
    # ... and the same ranking, up to the order inside groups of genes whose values agree to RTOL (two rare genes with one
    # multiset of counts have one standardised variance up to the rounding of a sum over different cells)
    assert np.array_equal(feats.genes, preprocess.top_features(feats.variance_standardized, ref.PLANTED_FEATURES))
    close(vs[feats.genes], vs[genes])


# ---- 7. end to end --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_groups_end_to_end(seed):
    X, groups = ref.planted_counts(seed)
    n = X.shape[0]
    emb = preprocess.embed(X, nfeatures=ref.PLANTED_FEATURES, npcs=ref.PLANTED_PCS)
    assert emb.coords.shape == (n, ref.PLANTED_PCS) and len(emb.genes) == ref.PLANTED_FEATURES
    assert emb.features.variance_standardized.shape == (X.shape[1],)
    g = snn.build_snn(emb.coords[:, :3], k=10)
    rows = np.repeat(np.arange(n), np.diff(g.rowptr))
    assert len(g.col) > 0 and np.array_equal(groups[rows], groups[g.col])      # no edge joins two planted groups
    labels, counts = metrics.connected_components((g.rowptr, g.col), n)
    assert counts[0] >= 4
    for c in range(int(counts[0])):
        assert len(set(groups[labels[0] == c].tolist())) == 1
    if seed == 0:
        Y = preprocess.log_normalize(X)
        assert Y.shape == X.shape and Y.dtype == np.float32
        mk = metrics.find_all_markers(Y, groups)
        assert mk["p_val"].shape == (X.shape[1], 4)
        planted = np.arange(40)                                  # group 0's genes are its markers
        assert np.all(mk["avg_log2FC"][planted, 0] > 0.5)


# ---- 8. errors ------------------------------------------------------------------------------------------------------------

def code_of(fn, *args):
    with pytest.raises(_lib.MiSaError) as ei:
        fn(*args)
    return ei.value.code


def test_errors():
    X = ref.sparse_counts(np.random.default_rng(8), 10, 6)
    for bad in (np.nan, -1.0, np.inf):
        B = X.copy()
        B[3, 2] = bad
        assert code_of(ExpressionMatrix, B) == EINVAL
    assert code_of(ExpressionMatrix, X[:1]) == EINVAL
    with ExpressionMatrix(X) as m:
        one = np.ones(3)
        assert code_of(m.fetch_normalized) == ESTATE
        assert code_of(m.gene_stats, "normalized") == ESTATE
        assert code_of(m.select, [0, 1, 2], one, one) == ESTATE
        assert code_of(m.gram) == ESTATE
        assert code_of(m.normalize, 0.0) == EINVAL
        m.normalize()
        assert code_of(m.fetch_scaled) == ESTATE
        assert code_of(m.select, [0, 1, 1], one, one) == EINVAL                  # duplicate
        assert code_of(m.select, [0, 1, 6], one, one) == EINVAL                  # out of range
        assert code_of(m.select, [0, -1, 2], one, one) == EINVAL
        assert code_of(m.select, [0, 1, 2], one, -one) == EINVAL
        assert code_of(m.select, [0, 1, 2], one, one, 0.0) == EINVAL
        big = np.ones(4097)
        assert code_of(m.select, np.zeros(4097, dtype=np.int32), big, big) == EUNSUPPORTED
        assert code_of(m.gram) == ESTATE                                         # a failed select leaves nothing selected
        m.select([0, 1, 2], one, one)
        assert code_of(m.project, np.ones((3, 129), dtype=np.float32)) == EUNSUPPORTED
        assert code_of(m.project, np.full((3, 2), np.nan, dtype=np.float32)) == EINVAL
        assert code_of(m.clipped_variance, np.zeros(6), -np.ones(6), 3.0) == EINVAL
        with pytest.raises(ValueError):
            m.project(np.ones((4, 2)))
        with pytest.raises(ValueError):
            preprocess.pca(m, [0, 1, 2], npcs=4)
        with pytest.raises(ValueError):
            preprocess.find_variable_features(m, nfeatures=7)
        assert m.project(np.ones((3, 2))).shape == (10, 2)                       # the handle survives all of it
