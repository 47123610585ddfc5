"""Host side of UMAP (scrna_seq_qannealing_clustering_amd/umap.py) and the numpy reference of chain U
(tests/umap_reference.py), without a GPU: the reference's Philox against the oracle's, the curve constants against the
published umap-learn / Seurat values, the PCA initialisation's edges, the firing schedule, the smooth-kNN normalisation
of the reference, every argument error of the Python layer (raised before any ctypes call), and the embedding plot."""
import hashlib
import os

import numpy as np
import pytest

import umap_layout_cases as uc
import umap_reference as ref
from oracle import sa_oracle as so
from scrna_seq_qannealing_clustering_amd import metrics, outputs, umap


def test_numpy_philox_equals_the_oracle():
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 2 ** 32, size=(300, 4), dtype=np.uint64)
    ctr[:4] = [[0, 0, 0, 0], [2 ** 32 - 1] * 4, [1, 0, 0, 0], [0, 0, 0, 1]]
    for key in ((0, 0), (42, 0), (0xFFFFFFFF, 0xFFFFFFFF), (0x12345678, 0x9ABCDEF0)):
        got = np.stack(ref.philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], *key), axis=1)
        want = np.array([so.philox4x32_10([int(v) for v in row], key) for row in ctr], dtype=np.uint32)
        assert np.array_equal(got, want)


def test_find_ab_params_published_values():
    np.testing.assert_allclose(umap.find_ab_params(1.0, 0.1), (1.577, 0.8951), rtol=1e-3)
    np.testing.assert_allclose(umap.find_ab_params(1.0, 0.3), (0.9922, 1.112), rtol=1e-3)
    for bad in ((0.0, 0.1), (1.0, -0.1), (1.0, 2.0), (np.nan, 0.1), (1.0, np.inf)):
        with pytest.raises(ValueError):
            umap.find_ab_params(*bad)


def test_pca_init_edges():
    X = np.random.default_rng(1).normal(size=(40, 5)) * [3.0, 1.0, 7.0, 1.0, 1.0] + 100.0
    for c in (2, 3):
        Y = umap.pca_init(X, c)
        assert Y.shape == (40, c) and Y.dtype == np.float32
        assert abs(np.abs(Y).max() - 10.0) < 1e-6
        assert np.abs(Y.astype(np.float64).mean(axis=0)).max() < 1e-5
        Z = X[:, :c] - X[:, :c].mean(axis=0)                       # one common factor: the columns keep their ratio
        np.testing.assert_allclose(Y, Z * (10.0 / np.abs(Z).max()), rtol=1e-6, atol=1e-6)
    assert not umap.pca_init(np.full((5, 2), 3.0), 2).any()      # constant columns: zeros, no division by zero
    for bad in (np.ones((5, 1)), np.ones(5), np.full((5, 2), np.nan)):
        with pytest.raises(ValueError):
            umap.pca_init(bad, 2)
    with pytest.raises(ValueError):
        umap.pca_init(np.ones((5, 4)), 4)
    assert umap.default_n_epochs(10000) == 500 and umap.default_n_epochs(10001) == 200


def test_firing_schedule_counts():
    for T in (1, 8, 200, 500):
        for p in (1.0, 0.5, 1.0 / 3.0, 0.9 / T, 1.0 / T, 0.123456, 0.999, 1e-9):
            p32 = np.float32(p)
            assert ref.fire_counts(p32, T) == int(np.floor(np.float32(T) * p32)), (T, p)


def test_reference_smooth_normalises_to_log2_k():
    rng = np.random.default_rng(2)
    X = rng.normal(size=(200, 6)).astype(np.float32)
    for k in (2, 5, 15, 64):
        nn = ref.knn_exact(X, k)
        dist = ref.distances(X, nn, "euclidean")
        rho, sigma, binds, _ = ref.smooth(dist)
        assert np.array_equal(rho, dist[:, 1].astype(np.float64)) and (~binds).sum() > 100
        x = dist[:, 1:].astype(np.float64) - rho[:, None]
        v = np.where(x <= 0, 1.0, np.exp(-x / sigma[:, None]))
        assert np.abs(v.sum(axis=1) - np.log2(k))[~binds].max() < 1e-9
    # the reference's U3 is symmetric with rows ascending, and its distances restate the brute force
    rowptr, col, w64, w32 = ref.union(nn, dist, rho, sigma)
    rows = np.repeat(np.arange(200), np.diff(rowptr))
    M = np.zeros((200, 200), dtype=np.float32)
    M[rows, col] = w32
    assert np.array_equal(M, M.T) and not M.diagonal().any() and w32.min() > 0 and w32.max() <= 1.0
    d64 = np.sqrt(((X[:, None, :].astype(np.float64) - X[nn].astype(np.float64)) ** 2).sum(axis=2))
    np.testing.assert_allclose(dist, d64, rtol=1e-5)


def test_reference_layout_float32_tracks_fp64():
    rowptr, col, w = ref.handmade_graph()
    Y0 = (np.random.default_rng(3).normal(size=(len(rowptr) - 1, 2)) * 4.0).astype(np.float32)
    y64 = ref.layout(rowptr, col, w, Y0, 1.577, 0.8951, 1.0, 8, 0, 42, np.float64)
    y32 = ref.layout(rowptr, col, w, Y0, 1.577, 0.8951, 1.0, 8, 0, 42, np.float32)
    assert y32.dtype == np.float32 and 0 < np.abs(y32 - y64).max() < 1e-4
    # with negatives the two trajectories part further (a repulsion near s = 0 is steep), and another seed is another run
    n5 = [ref.layout(rowptr, col, w, Y0, 1.577, 0.8951, 1.0, 8, 5, seed, np.float64) for seed in (42, 43)]
    assert np.isfinite(n5[0]).all() and not np.array_equal(n5[0], n5[1]) and not np.array_equal(n5[0], y64)
    assert np.abs(y64 - Y0).max() > 0.5                            # the points did move
    assert np.array_equal(y64[50], Y0[50].astype(np.float64))      # the empty row


def test_reference_layout_default_path_is_unchanged():
    """`mutate=None` is the function as it was before `mutate` existed: the stored hashes are the old function's results.
    a = b = 1: pow(s, 1) and pow(s, 0) are exact in every libm, so the bits depend on numpy's +, -, *, / alone, while the run
    still passes every line a mutation touches (schedule, alpha, Philox addressing, self-draws, 0.001, clamp)."""
    rowptr, col, w = ref.handmade_graph()
    Y0 = (np.random.default_rng(3).normal(size=(203, 3)) * 4.0).astype(np.float32)
    want = {np.float64: "957183b472ef93c61ca18b907bc714c0189af1e9fc8f0996999ed5677da21557",
            np.float32: "f837e6289e83855ea08f0bbb386761044cf2d8d7913fd470d867118ba65454ec"}
    for dt, digest in want.items():
        y = ref.layout(rowptr, col, w, Y0, 1.0, 1.0, 1.0, 8, 5, 2 ** 40 + 42, dt)
        assert hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest() == digest
    with pytest.raises(AssertionError):
        ref.layout(rowptr, col, w, Y0, 1.0, 1.0, 1.0, 8, 5, 42, mutate="no such line")


def test_graph_builders():
    for name, (_, lanes, mean) in uc.GRAPHS.items():
        rowptr, col, w = uc.graph(name)                            # (asserts the mean, the empty row, the long row, max w = 1)
        n = len(rowptr) - 1
        rows = np.repeat(np.arange(n), np.diff(rowptr))
        M = np.zeros((n, n), dtype=np.float32)
        M[rows, col] = w
        assert not M.diagonal().any() and (np.diff(col)[np.diff(rows) == 0] > 0).all()
        odd = int(rowptr[-1]) & 1                                  # an odd number of entries: exactly one has no mirror
        assert ((M > 0) != (M.T > 0)).sum() == 2 * odd and np.array_equal(M[(M > 0) & (M.T > 0)], M.T[(M > 0) & (M.T > 0)])
    assert uc.graph("mean16")[0][-1] == 16 * 67 and uc.graph("mean32+")[0][-1] == 32 * 67 + 1
    for T in (8, 10000):
        rowptr, col, w, edges = ref.schedule_graph(T)
        assert w.max() == 1.0 and np.diff(rowptr)[7] == 1 and col[-1] == 6 and col[rowptr[7] - 1] == 7
        assert ref.fire_counts(edges[6, 7], T) == 0 and ref.fire_counts(edges[4, 5], T) == 1
        assert ref.fire_counts(edges[0, 1], T) == T and ref.fire_counts(edges[1, 2], T) == T - 1


# which deviations a case can show at all: without negatives nothing is drawn
NEEDS_NEG = ("philox_t_q", "philox_local_E", "keep_self", "no_eps")


@pytest.mark.parametrize("group", ["g16", "g32", "g64", "mean"])
def test_small_step_criterion_sees_errors(group):
    """The conditions tests/test_gpu_umap_layout.py relies on, shown on the reference alone for every one of its cases:
    D32 is storage rounding (<= 8 f32 steps of the largest coordinate; observed: at most 2.65 steps on the x4 starts, at most
    6.87 on the x0.5 starts -- above 3 only at neg = 16, where a vertex moves up to 1.0), the largest move is >= 1000 D32
    (observed: >= 3978), and every deviation of ref.MUTATIONS that changes the fp64 result at all changes it by more than
    the 4 D32 the device is allowed.  Smallest observed (change / D32) over the cases where the deviation acts, x4 / x0.5 start:
        philox_t_q 484 / 64931      philox_local_E 485 / 47848     fire_next 1112 / 49370      alpha_next 983 / 20230
        keep_self 1539 / 15141      clamp_coef 5.4 / 501           no_eps 0.28 / 880
    no_eps is asserted on the x0.5 starts only.  Leaving 0.001 out changes a repulsive term by the factor 0.001 / s; on the
    x4 starts a drawn pair has s of the order 2 * c * 16 >= 64, the term itself is below 2 b / s^1.5, and 8 epochs of
    2^-10 of that are below the rounding of a coordinate near 10: there the criterion cannot see it, which is why the cases
    have a second start with s of the order 1.  clamp_coef acts without negatives too (an attraction at s < 1, b < 1)."""
    seen = {}                                                     # mutation -> smallest change / D32
    for case in uc.CASES:
        g, c, neg, scale, seed, ab = case
        if not g.startswith(group):
            continue
        rowptr, col, w, Y0, y64, d32, moved = uc.reference(case)
        top = np.abs(Y0).max() if scale == 0.5 else np.abs(y64).max()
        assert 0.0 < d32 <= 8.0 * np.spacing(np.float32(top)), uc.case_id(case)
        assert moved >= 1000.0 * d32, uc.case_id(case)
        for m in ref.MUTATIONS:
            if neg == 0 and m in NEEDS_NEG:
                continue
            ym = ref.layout(rowptr, col, w, Y0, *uc.AB[ab], uc.LR, uc.T8, neg, seed, np.float64, mutate=m)
            change = float(np.abs(ym - y64).max())
            if change == 0.0:                                     # cannot act here (no self-draw, no term beyond the clamp)
                assert m in ("keep_self", "clamp_coef"), (m, uc.case_id(case))
                continue
            if m == "no_eps" and scale != 0.5:
                continue
            assert change > 4.0 * d32, (m, uc.case_id(case), change / d32)
            seen[m] = min(seen.get(m, np.inf), change / d32)
    # every deviation acted, and was seen, in this group alone
    assert set(seen) == set(ref.MUTATIONS), sorted(set(ref.MUTATIONS) - set(seen))


def test_python_argument_errors(monkeypatch):
    from scrna_seq_qannealing_clustering_amd import _lib

    def no_library(*a, **k):
        raise AssertionError("an argument error must be raised before the library is touched")
    monkeypatch.setattr(_lib, "load", no_library)
    X = np.random.default_rng(4).normal(size=(20, 4)).astype(np.float32)
    bad_points = [
        dict(X=X[0]), dict(X=X[:1]), dict(X=np.zeros((20, 65), dtype=np.float32)), dict(X=np.zeros((20, 0))),
        dict(X=np.where(np.arange(80).reshape(20, 4) == 7, np.nan, X)), dict(X=X.astype(str)),
        dict(n_neighbors=1), dict(n_neighbors=21), dict(n_neighbors=65, X=np.zeros((70, 2))), dict(n_neighbors=2.5),
        dict(metric="manhattan"),
    ]
    for kw in bad_points:
        args = dict(X=X, n_neighbors=5, metric="euclidean")
        args.update(kw)
        with pytest.raises(ValueError):
            umap.knn(args["X"], args["n_neighbors"], args["metric"])
        with pytest.raises(ValueError):
            umap.fuzzy_graph(args["X"], args["n_neighbors"], args["metric"])
        with pytest.raises(ValueError):
            umap.run_umap(args["X"], n_neighbors=args["n_neighbors"], metric=args["metric"])
    for kw in (dict(n_components=1), dict(n_components=4), dict(n_epochs=0), dict(n_epochs=10001), dict(n_epochs=1.5),
               dict(negative_sample_rate=-1), dict(negative_sample_rate=17), dict(learning_rate=0.0),
               dict(learning_rate=np.nan), dict(seed=-1), dict(seed=2 ** 64), dict(min_dist=-1.0), dict(min_dist=2.0),
               dict(spread=0.0), dict(init="spectral"), dict(init=np.zeros((19, 2))), dict(init=np.zeros((20, 3))),
               dict(init=np.full((20, 2), np.inf)), dict(n_components=3, X=X[:, :2], init="pca")):
        args = dict(X=X, n_neighbors=5)
        args.update(kw)
        with pytest.raises(ValueError):
            umap.run_umap(**args)
    rowptr, col, w = np.array([0, 1, 2]), np.array([1, 0]), np.array([1.0, 1.0])
    Y0 = np.zeros((2, 2), dtype=np.float32)
    for kw in (dict(rowptr=np.array([0.0, 1.0, 2.0])), dict(rowptr=np.array([0])), dict(col=np.array([1])),
               dict(w=np.array([1.0])), dict(col=np.array([1.0, 0.0])), dict(col=np.array([2 ** 31, 0])),
               dict(init=np.zeros((3, 2))), dict(init=np.zeros(2)), dict(a=np.inf), dict(b=np.nan), dict(n_epochs=0),
               dict(negative_sample_rate=17), dict(learning_rate=-1.0), dict(seed=-5)):
        args = dict(rowptr=rowptr, col=col, w=w, init=Y0, a=1.0, b=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            umap.layout(**args)
    for bad in (dict(nn_high=np.zeros((5, 1), dtype=int)), dict(nn_high=np.zeros((5, 3))), dict(Y=np.zeros((4, 2))),
                dict(k=1), dict(k=4)):
        args = dict(nn_high=np.zeros((5, 3), dtype=np.int32), Y=np.zeros((5, 2)), k=None)
        args.update(bad)
        with pytest.raises(ValueError):
            metrics.knn_preservation(**args)


def test_normalize_rows_matches_the_reference():
    X = np.random.default_rng(5).normal(size=(33, 7)).astype(np.float32)
    X[4] = 0.0
    U = umap.normalize_rows(X)
    assert np.array_equal(U, ref.normalize_rows(X)) and not U[4].any()
    np.testing.assert_allclose(np.linalg.norm(np.delete(U, 4, axis=0), axis=1), 1.0, rtol=1e-6)


def test_plot_and_save_embedding_writes_a_file(tmp_path):
    pytest.importorskip("matplotlib")
    rng = np.random.default_rng(6)
    coords = rng.normal(size=(60, 2)).astype(np.float32)
    labels = np.arange(60) % 3
    path = str(tmp_path / "sub" / "umap.png")
    assert outputs.plot_and_save_embedding(coords, labels, path, title="clusters") == [0, 1, 2]
    assert os.path.getsize(path) > 0
    path2 = str(tmp_path / "plain.png")
    assert outputs.plot_and_save_embedding(rng.normal(size=(10, 3)), None, path2) == [0]
    assert os.path.getsize(path2) > 0
    assert outputs.plot_and_save_embedding(coords, np.array(["a", "b"] * 30), str(tmp_path / "s.png")) == ["a", "b"]
    with pytest.raises(ValueError):
        outputs.plot_and_save_embedding(coords, labels[:5], path)
    with pytest.raises(ValueError):
        outputs.plot_and_save_embedding(coords[:, :1], None, path)
