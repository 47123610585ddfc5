"""The host side of the preprocessing front end (``preprocess.py``), no GPU: ``loess_fit`` against exact polynomials and a
brute-force weighted least-squares fit, ``pca_from_gram`` against ``np.linalg.svd``, argument validation (the native
checks run before any device work, so they are reachable here), the tie order of the feature ranking, and the condition
the end-to-end GPU test (tests/test_gpu_prep.py) relies on, checked with the numpy reference alone: on the planted
matrix every cell's 9 nearest other cells in the first 3 reference PCs belong to its own group."""
import ctypes

import numpy as np
import pytest

import prep_reference as ref
from scrna_seq_qannealing_clustering_amd import _lib, preprocess
from scrna_seq_qannealing_clustering_amd.preprocess import loess_fit, pca_from_gram, top_features


# ---- loess_fit -----------------------------------------------------------------------------------------------------------

def test_loess_reproduces_a_quadratic():
    rng = np.random.default_rng(0)
    x = rng.uniform(-2.0, 3.0, 200)
    y = 0.7 - 1.3 * x + 0.45 * x * x
    for span in (0.1, 0.3, 1.0):
        assert np.abs(loess_fit(x, y, span=span, degree=2) - y).max() <= 1e-10
    line = 2.0 + 0.5 * x
    assert np.abs(loess_fit(x, line, span=0.3, degree=1) - line).max() <= 1e-10


def brute_force_fit(x, y, i, span, degree):
    m = len(x)
    q = min(m, int(np.ceil(span * m)))
    dist = np.abs(x - x[i])
    near = np.argsort(dist, kind="stable")[:q]
    d = dist[near].max()
    w = (1.0 - (dist[near] / d) ** 3) ** 3
    A = np.vander(x[near] - x[i], degree + 1, increasing=True)
    sw = np.sqrt(w)
    return np.linalg.lstsq(A * sw[:, None], y[near] * sw, rcond=None)[0][0]


@pytest.mark.parametrize("span, degree", [(0.3, 2), (0.15, 1), (0.5, 2), (1.0, 2)])
def test_loess_equals_brute_force(span, degree):
    rng = np.random.default_rng(1)
    x = rng.normal(0.0, 1.0, 150)
    y = np.sin(2.0 * x) + 0.3 * rng.normal(size=150)
    fit = loess_fit(x, y, span=span, degree=degree)
    for i in rng.permutation(150)[:20]:
        want = brute_force_fit(x, y, i, span, degree)
        assert abs(fit[i] - want) <= 1e-9 * max(1.0, abs(want)), (i, fit[i], want)


def test_loess_span_one_uses_all_points():
    rng = np.random.default_rng(2)
    x = np.sort(rng.uniform(0.0, 1.0, 40))
    y = rng.normal(size=40)
    base = loess_fit(x, y, span=1.0, degree=2)
    assert np.array_equal(loess_fit(x, y, span=5.0, degree=2), base)
    # the end points' fits see the far end: moving the last y changes the first fit (a window of 39 would not reach it ...
    y2 = y.copy()
    y2[-2] += 1.0
    assert loess_fit(x, y2, span=1.0, degree=2)[0] != base[0]
    # ... while the farthest point itself carries weight 0)
    y3 = y.copy()
    y3[-1] += 1.0
    assert abs(loess_fit(x, y3, span=1.0, degree=2)[0] - base[0]) <= 1e-12


def test_loess_ties_and_validation():
    x = np.array([1.0] * 6 + [2.0, 3.0, 4.0, 5.0])
    y = np.arange(10.0)
    fit = loess_fit(x, y, span=0.3, degree=2)                    # q = 3: the windows of the tied points hold x = 1 only
    assert np.allclose(fit[:6], 1.0)                             # the mean of the first three y
    with pytest.raises(ValueError):
        loess_fit(x, y[:5])
    with pytest.raises(ValueError):
        loess_fit(x, y, span=0.0)
    with pytest.raises(ValueError):
        loess_fit(x, y, degree=3)
    with pytest.raises(ValueError):
        loess_fit(x, y, span=0.1, degree=2)                      # one point per window
    with pytest.raises(ValueError):
        loess_fit(np.array([0.0, np.nan, 1.0]), np.zeros(3), span=1.0)


# ---- pca_from_gram -------------------------------------------------------------------------------------------------------

def test_pca_from_gram_against_svd():
    rng = np.random.default_rng(3)
    n, h, npcs = 300, 40, 12
    Z = rng.normal(size=(n, h)) * rng.uniform(0.5, 3.0, h)
    G = Z.T @ Z
    r = pca_from_gram(G, n, npcs)
    sv = np.linalg.svd(Z, compute_uv=False)
    want = sv[:npcs] ** 2 / (n - 1)
    assert np.abs(r.eigenvalues - want).max() <= 1e-10 * want[0]
    assert np.all(np.abs(r.eigenvalues - want) <= 1e-10 * want)
    assert np.all(np.diff(r.eigenvalues) <= 0)
    assert np.allclose(r.stdev, np.sqrt(want), rtol=1e-10)
    assert abs(r.total_variance - (sv ** 2).sum() / (n - 1)) <= 1e-10 * r.total_variance
    V = r.loadings
    assert V.shape == (h, npcs)
    assert np.abs(V.T @ V - np.eye(npcs)).max() <= 1e-10
    resid = np.linalg.norm(G / (n - 1) @ V - V * r.eigenvalues, axis=0)
    assert resid.max() <= 1e-10 * r.eigenvalues[0]
    top = np.argmax(np.abs(V), axis=0)
    assert np.all(V[top, np.arange(npcs)] > 0)


def test_pca_sign_rule_takes_the_first_of_equal_magnitudes():
    # eigenvectors (1, -1)/sqrt 2 and (1, 1)/sqrt 2: both entries tie in magnitude, the first one decides
    r = pca_from_gram(np.array([[2.0, -1.0], [-1.0, 2.0]]), 2, 2)
    assert np.allclose(r.eigenvalues, [3.0, 1.0])
    assert np.all(r.loadings[0] > 0)
    assert r.loadings[1, 0] < 0 < r.loadings[1, 1]


def test_pca_from_gram_validation():
    G = np.eye(4)
    for bad in (0, 5):
        with pytest.raises(ValueError):
            pca_from_gram(G, 10, bad)
    with pytest.raises(ValueError):
        pca_from_gram(np.ones((3, 4)), 10, 2)
    with pytest.raises(ValueError):
        pca_from_gram(G, 1, 2)


# ---- feature ranking and argument validation ------------------------------------------------------------------------------

def test_top_features_stable_ties():
    vs = np.array([1.0, 3.0, 2.0, 3.0, 0.0, 2.0, 3.0])
    assert top_features(vs, 5).tolist() == [1, 3, 6, 2, 5]
    assert top_features(vs, 2).tolist() == [1, 3]
    assert top_features(np.zeros(4), 3).tolist() == [0, 1, 2]
    assert top_features(vs, 7).dtype == np.int32
    for bad in (0, 8):
        with pytest.raises(ValueError):
            top_features(vs, bad)
    with pytest.raises(ValueError):
        top_features(np.array([1.0, np.nan]), 1)


def test_expected_sd_skips_constant_genes():
    rng = np.random.default_rng(4)
    mean = rng.uniform(0.1, 5.0, 60)
    var = mean * (1.0 + 0.3 * mean)
    var[[3, 17]] = 0.0
    sd = preprocess.expected_sd_from_stats(mean, var, span=0.5)
    assert sd[3] == 0.0 and sd[17] == 0.0
    ok = var > 0
    assert np.allclose(sd[ok] ** 2, var[ok], rtol=0.05)          # a smooth curve is recovered


def test_native_argument_checks_precede_device_work():
    lib = _lib.load()
    h = ctypes.c_void_p()
    f32p = ctypes.POINTER(ctypes.c_float)

    def create(X):
        X = np.ascontiguousarray(X, dtype=np.float32)
        return lib.mi_prep_create_f32(X.ctypes.data_as(f32p), X.shape[0], X.shape[1], 0, ctypes.byref(h))

    assert create(np.ones((1, 3))) == -1 and b"n must be" in lib.mi_last_error()
    bad = np.ones((4, 3))
    for v in (np.nan, np.inf, -1.0):
        bad[2, 1] = v
        assert create(bad) == -1 and b"X[2, 1]" in lib.mi_last_error()
    assert lib.mi_prep_create_f32(None, 4, 3, 0, ctypes.byref(h)) == -1
    assert lib.mi_prep_create_f32(bad.astype(np.float32).ctypes.data_as(f32p), 4, 0, 0, ctypes.byref(h)) == -1
    assert lib.mi_prep_create_f32(bad.astype(np.float32).ctypes.data_as(f32p), (1 << 23) + 1, 1, 0, ctypes.byref(h)) == -5
    assert lib.mi_prep_create_f32(bad.astype(np.float32).ctypes.data_as(f32p), 1 << 20, 1 << 13, 0, ctypes.byref(h)) == -5
    assert lib.mi_prep_normalize(None, 1e4, None) == -1
    assert lib.mi_prep_destroy(None) == 0
    with pytest.raises(ValueError):
        preprocess.ExpressionMatrix(np.ones(5))
    with pytest.raises(_lib.MiSaError) as ei:
        preprocess.ExpressionMatrix(np.ones((1, 5)))
    assert ei.value.code == -1


def test_module_is_exported():
    import scrna_seq_qannealing_clustering_amd as pkg
    assert pkg.preprocess is preprocess and "preprocess" in pkg.__all__


# ---- the condition behind the end-to-end GPU test -------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_groups_separate_in_the_reference(seed):
    X, groups = ref.planted_counts(seed)
    coords, w, genes = ref.pca_coords(X, ref.PLANTED_FEATURES, ref.PLANTED_PCS, loess_fit)
    assert len(set(genes.tolist())) == ref.PLANTED_FEATURES
    P = coords[:, :3]
    D = ((P[:, None, :] - P[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(D, np.inf)
    near = np.argsort(D, axis=1, kind="stable")[:, :9]
    purity = (groups[near] == groups[:, None]).mean()
    print("seed %d: purity %.4f, leading eigenvalues %s, bulk %.2f" % (seed, purity, np.round(w[:5], 2), w[5]))
    assert purity == 1.0
    assert w[2] > 2.0 * w[4]                                     # three planted directions stand clear of the bulk
