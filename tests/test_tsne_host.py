"""Chain T without a GPU: what the C ABI refuses (every check runs before any device work), the numpy reference on its own,
and that the small-step criterion of tests/test_gpu_tsne.py can see the mistakes a t-SNE layout is likely to make."""
import ctypes as C

import numpy as np
import pytest

import tsne_cases as tc
import tsne_reference as ref
from scrna_seq_qannealing_clustering_amd import _lib, tsne

EINVAL, EUNSUPPORTED = -1, -5                                 # MI_EINVAL, MI_EUNSUPPORTED of include/mi_sa.h


def code(name, *args):
    with pytest.raises(_lib.MiSaError) as ei:
        _lib.call(name, *args)
    return ei.value.code


# ---- ABI refusals -----------------------------------------------------------------------------------------------------------------

def knn_args(X=None, n=None, dim=None, perplexity=2.0, out=True):
    X = np.random.default_rng(0).normal(size=(40, 3)).astype(np.float32) if X is None else X
    return (X, X.shape[0] if n is None else n, X.shape[1] if dim is None else dim, perplexity, 0,
            C.c_void_p() if out else None, None)


def test_knn_refusals():
    X = np.random.default_rng(0).normal(size=(40, 3)).astype(np.float32)
    assert code("mi_tsne_knn_f32", None, 40, 3, 2.0, 0, C.c_void_p(), None) == EINVAL
    assert code("mi_tsne_knn_f32", *knn_args(out=False)) == EINVAL
    for perplexity in (1.999, 85.001, float("nan"), float("inf"), -1.0):
        assert code("mi_tsne_knn_f32", *knn_args(perplexity=perplexity)) == EINVAL, perplexity
    # 3 * perplexity > n - 1: n = 40 holds K = 39 (perplexity 13) and not K = 40
    assert code("mi_tsne_knn_f32", *knn_args(perplexity=13.34)) == EINVAL
    assert b"perplexity is too large" in _lib.load().mi_last_error()
    assert code("mi_tsne_knn_f32", *knn_args(np.zeros((255, 1), dtype=np.float32), perplexity=85.0)) == EINVAL   # K = 255 = n
    assert code("mi_tsne_knn_f32", *knn_args(dim=0)) == EINVAL
    assert code("mi_tsne_knn_f32", *knn_args(np.zeros((40, 65), dtype=np.float32))) == EINVAL
    assert code("mi_tsne_knn_f32", *knn_args(n=1)) == EINVAL
    bad = X.copy()
    bad[17, 2] = np.nan
    assert code("mi_tsne_knn_f32", *knn_args(bad)) == EINVAL
    assert b"X[17, 2]" in _lib.load().mi_last_error()
    wide = X.copy()
    wide[0, 0], wide[1, 0] = 3e38, -3e38                           # the coordinate-range rule of mi_snn.h
    assert code("mi_tsne_knn_f32", *knn_args(wide)) == EINVAL
    big = np.zeros(((1 << 18) + 1, 1), dtype=np.float32)
    assert code("mi_tsne_knn_f32", *knn_args(big)) == EUNSUPPORTED
    for name, args in (("mi_tsne_fetch_knn", (None, None, None)), ("mi_tsne_calibrate", (None, None)),
                       ("mi_tsne_fetch_calibration", (None, None, None)), ("mi_tsne_symmetrize", (None, None)),
                       ("mi_tsne_info", (None, None, None, None, None)), ("mi_tsne_fetch_graph", (None, None, None, None))):
        assert code(name, *args) == EINVAL, name
    assert _lib.call("mi_tsne_destroy", None) == 0


def layout_args(**kw):
    rowptr = np.array([0, 1, 3, 4], dtype=np.int64)
    col = np.array([1, 0, 2, 1], dtype=np.int32)
    P = np.array([0.25, 0.25, 0.25, 0.25], dtype=np.float32)
    Y = np.arange(6, dtype=np.float32).reshape(3, 2)
    a = dict(n=3, c=2, rowptr=rowptr, col=col, P=P, Y=Y, U=None, gains=None, eta=200.0, exag=12.0, exag_iters=250, m0=0.5,
             m1=0.8, switch=250, T=10, t0=0, center=1, device=0, Y_out=np.empty_like(Y), U_out=None, gains_out=None, Z_out=None)
    a.update(kw)
    return tuple(a.values()) + (None,)


def kl_args(**kw):
    a = layout_args(**kw)
    return a[:6] + (0, kw.get("kl", C.c_double(0.0)), None)


def test_layout_refusals():
    assert code("mi_tsne_layout_f32", *layout_args(rowptr=None)) == EINVAL
    assert code("mi_tsne_layout_f32", *layout_args(Y=None)) == EINVAL
    assert code("mi_tsne_layout_f32", *layout_args(Y_out=None)) == EINVAL
    assert code("mi_tsne_layout_f32", *layout_args(col=None)) == EINVAL
    assert code("mi_tsne_layout_f32", *layout_args(P=None)) == EINVAL
    Y4 = np.zeros((3, 4), dtype=np.float32)
    assert code("mi_tsne_layout_f32", *layout_args(c=4, Y=Y4, Y_out=Y4.copy())) == EUNSUPPORTED
    assert code("mi_tsne_layout_f32", *layout_args(c=1)) == EUNSUPPORTED
    for T in (0, -1, 10001):
        assert code("mi_tsne_layout_f32", *layout_args(T=T)) == EINVAL, T
    assert code("mi_tsne_layout_f32", *layout_args(t0=-1)) == EINVAL
    assert code("mi_tsne_layout_f32", *layout_args(n=1, rowptr=np.array([0, 0], dtype=np.int64))) == EINVAL
    # a diagonal entry, a descending row, a column outside [0, n), a decreasing rowptr, rowptr[0] != 0
    assert code("mi_tsne_layout_f32", *layout_args(col=np.array([1, 1, 2, 1], dtype=np.int32))) == EINVAL
    assert b"diagonal" in _lib.load().mi_last_error()
    assert code("mi_tsne_layout_f32", *layout_args(col=np.array([1, 2, 0, 1], dtype=np.int32))) == EINVAL
    assert b"ascending" in _lib.load().mi_last_error()
    assert code("mi_tsne_layout_f32", *layout_args(col=np.array([1, 0, 3, 1], dtype=np.int32))) == EINVAL
    assert code("mi_tsne_layout_f32", *layout_args(rowptr=np.array([0, 3, 1, 4], dtype=np.int64))) == EINVAL
    assert code("mi_tsne_layout_f32", *layout_args(rowptr=np.array([1, 1, 3, 4], dtype=np.int64))) == EINVAL
    for w in (0.0, -0.25, np.nan, np.inf):
        assert code("mi_tsne_layout_f32", *layout_args(P=np.array([0.25, w, 0.25, 0.25], dtype=np.float32))) == EINVAL, w
    bad = np.arange(6, dtype=np.float32).reshape(3, 2)
    bad[2, 1] = np.inf
    assert code("mi_tsne_layout_f32", *layout_args(Y=bad)) == EINVAL
    assert code("mi_tsne_layout_f32", *layout_args(U=bad)) == EINVAL
    assert code("mi_tsne_layout_f32", *layout_args(gains=bad)) == EINVAL
    assert code("mi_tsne_layout_f32", *layout_args(gains=np.zeros((3, 2), dtype=np.float32))) == EINVAL
    for kw in (dict(eta=np.nan), dict(exag=np.inf), dict(m0=np.nan), dict(m1=np.inf)):
        assert code("mi_tsne_layout_f32", *layout_args(**kw)) == EINVAL, kw


def test_kl_refusals():
    assert code("mi_tsne_kl_f32", *kl_args(kl=None)) == EINVAL
    assert code("mi_tsne_kl_f32", *kl_args(Y=None)) == EINVAL
    assert code("mi_tsne_kl_f32", *kl_args(c=4)) == EUNSUPPORTED
    assert code("mi_tsne_kl_f32", *kl_args(col=np.array([1, 1, 2, 1], dtype=np.int32))) == EINVAL
    assert code("mi_tsne_kl_f32", *kl_args(col=np.array([1, 2, 0, 1], dtype=np.int32))) == EINVAL


def test_python_checks_come_before_the_library():
    X = np.random.default_rng(0).normal(size=(40, 3))
    for kw in (dict(perplexity=1.0), dict(perplexity=86), dict(perplexity=13.34), dict(n_components=4), dict(n_iter=0),
               dict(init="spectral"), dict(momentum=0.5), dict(learning_rate=0.0)):
        with pytest.raises(ValueError):
            tsne.run_tsne(X, **{"perplexity": 5, **kw})
    with pytest.raises(ValueError):
        tsne.run_tsne(np.zeros((40, 65)), perplexity=5)
    assert tsne.n_neighbors(30) == 90 and tsne.n_neighbors(85) == 255 and tsne.n_neighbors(2.4) == 7
    assert [tsne.chunks(n) for n in (2, 127, 128, 2638, 50000, 1 << 18)] == [1, 1, 2, 16, 16, 16]
    Y = tsne.random_init(50, 3, seed=1)
    assert Y.dtype == np.float32 and Y.shape == (50, 3)
    assert np.array_equal(Y, (1e-4 * np.random.default_rng(1).standard_normal((50, 3))).astype(np.float32))
    Yp = tsne.scaled_pca_init(X, 2)
    assert Yp.dtype == np.float32 and abs(float(Yp[:, 0].astype(np.float64).std()) - 1e-4) < 1e-9
    import scrna_seq_qannealing_clustering_amd as pkg
    assert pkg.tsne is tsne and pkg.run_tsne is tsne.run_tsne and "tsne" in pkg.__all__


# ---- the reference alone ------------------------------------------------------------------------------------------------------

def test_reference_calibration_hits_the_perplexity():
    rng = np.random.default_rng(3)
    X = rng.normal(size=(120, 5)).astype(np.float32)
    X[100:110] = X[100]                                            # ten copies of one point: for K = 9 their rows are K duplicates
    for perplexity in (3.0, 10.0, 30.0):
        K = int(3 * perplexity)
        nn, d2 = ref.knn_lexsort(X, K)
        beta, cond, H = ref.calibrate(d2, perplexity)
        flat = ~(d2 - d2[:, :1]).any(axis=1)
        # (K = 9: the ten copies, and any point whose nine nearest are nine of the copies -- equal distances, the same rule)
        assert flat[100:110].all() and flat.sum() < 20 if K <= 9 else not flat.any()
        assert np.allclose(np.exp(H[~flat]), perplexity, rtol=1e-9, atol=0.0)
        assert np.allclose(np.exp(H[flat]), K, rtol=1e-12) and (beta[flat] == 2.0 ** 100).all()
        assert np.allclose(cond[flat], 1.0 / K, rtol=1e-15)
        assert np.allclose(cond.sum(axis=1), 1.0, rtol=1e-12)
        rowptr, col, P64, P32 = ref.joint(nn, cond)
        assert abs(P64.sum() - 1.0) < 1e-6 and abs(float(P32.astype(np.float64).sum()) - 1.0) < 1e-6
        M = ref.dense(rowptr, col, P32)
        assert np.array_equal(M, M.T) and not M.diagonal().any()


def test_reference_layout_lowers_kl_on_blobs():
    X, labels = ref.blobs(seed=1, n=90, dim=10)
    rowptr, col, P = ref.affinities(X, 10.0)[4:]
    Y0 = tsne.random_init(90, 2, 1)
    Y = ref.layout(rowptr, col, P, Y0, 200.0, 12.0, 100, 0.5, 0.8, 100, 300)[0]
    assert ref.kl(rowptr, col, P, Y) < ref.kl(rowptr, col, P, Y0)
    assert np.abs(Y.mean(axis=0)).max() < 1e-6
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    assert (labels[d.argmin(axis=1)] == labels).all()


def test_reference_resume_is_one_run():
    case = ("g16", 2, 4.0)
    whole = tc.run(case, np.float64)
    Y3, U3, G3, _ = tc.run(case, np.float64, T=3, center=False)
    rest = tc.run(case, np.float64, T=5, t0=3, state=(U3, G3), Y0=Y3)
    # (the state passes through f32, as the device's does: the reference's fp64 state is not representable)
    assert all(np.allclose(a, b, rtol=1e-6, atol=1e-9) for a, b in zip(whole[:3], rest[:3]))


# ---- sharpness -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_small_step_criterion_sees_the_mistakes(case):
    """For every layout case: D32 > 0, the largest move is at least 1000 D32, and a reference run with the wrong exaggeration
    switch, the wrong momentum switch, Z over i < j only, the gain rule inverted or bhtsne's factor 4 added moves Y by at
    least 1000 D32 -- 250 times the bound the device is held to."""
    rowptr, col, P, Y0, y64, d32, moved = tc.reference(case)
    assert d32 > 0.0 and moved >= 1000.0 * d32
    for m in tc.MUTATIONS:
        wrong = float(np.abs(tc.run(case, np.float64, mutate=m)[0] - y64).max())
        print("%s %s: %.0f D32" % (tc.case_id(case), m, wrong / d32))
        assert wrong >= 1000.0 * d32, m


@pytest.mark.parametrize("case", tc.ONE_STEP, ids=tc.case_id)
def test_gain_comparison_cap(case):
    """The share of components whose gradient sign is rounding (|g64| < 4 |g32 - g64|, left out of the device's exact gains
    comparison) stays under 1 % on the reference alone, and the step from the chosen state is visible: >= 1000 D32."""
    Y, U, gains, y64, u64, want, unsure, d32y, d32u = tc.one_step(case)
    print("%s: %d of %d components unsure, D32(Y) %.3e, D32(U) %.3e" % (tc.case_id(case), unsure.sum(), unsure.size, d32y, d32u))
    assert unsure.mean() <= 0.01
    assert d32y > 0.0 and float(np.abs(y64 - Y).max()) >= 1000.0 * d32y
    assert (want >= np.float32(0.01)).all() and (want != gains).all()
