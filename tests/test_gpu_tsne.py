"""Chain T on the device (csrc/tsne_kernels.hip) against tests/tsne_reference.py: the multi-pass kNN at its pass edges, the
calibration and the joint P, every k_tsne_repulse<C> / k_tsne_update<G, C> form in small-step runs, one iteration from a chosen
state, resuming, determinism and an end-to-end run.

The layout criterion is the project's: |Y - y64| <= 4 D32, D32 the distance between the reference's float32 and fp64 runs of
the same input (tests/test_gpu_umap_layout.py).  tests/test_tsne_host.py shows on the reference alone that every case would
move by at least 1000 D32 under each of five likely mistakes.  Observed figures: DESIGN.md section 5d."""
import numpy as np
import pytest

import tsne_cases as tc
import tsne_reference as ref
from scrna_seq_qannealing_clustering_amd import snn, tsne

pytestmark = pytest.mark.gpu


def ulps(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert (a >= 0).all() and (b >= 0).all()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def perplexity_for(K):
    p = K / 3.0 if K % 3 == 0 else (K + 0.25) / 3.0
    assert tsne.n_neighbors(p) == K and 2.0 <= p <= 85.0
    return p


def knn(X, K):
    with tsne.Affinities(X, perplexity_for(K)) as g:
        assert g.K == K
        return g.fetch_knn()


# ---- T1 ------------------------------------------------------------------------------------------------------------------------

N_SET, DIM_SET = (7, 65, 257, 300), (1, 3, 50)               # the issue's grid, every (n, K) with K <= n - 1
LATTICE_SIDE = {1: 30, 3: 4, 50: 2}                           # small integers: exact f32 distances, many ties


@pytest.mark.parametrize("dim", DIM_SET)
@pytest.mark.parametrize("n,K", [(n, K) for n in N_SET for K in (6, 63) if K <= n - 1])
def test_knn_one_pass_is_the_snn_search(n, K, dim):
    """K <= 63: bit for bit the neighbours of k_knn (snn.build_snn with k = K + 1, the point itself in column 0), and the
    distances are ascending and the fp64 distances of those indices to rtol 1e-5 (the f32 chain: 3 dim roundings of 2^-24,
    9e-6 at dim = 50)."""
    X = np.random.default_rng(n * 100 + dim).normal(size=(n, dim)).astype(np.float32)
    nn, d2 = knn(X, K)
    assert nn.shape == d2.shape == (n, K) and nn.dtype == np.int32 and d2.dtype == np.float32
    assert np.array_equal(nn, snn.build_snn(X, K + 1).nn[:, 1:])
    assert (np.diff(d2, axis=1) >= 0).all() and (d2 >= 0).all()
    exact = ((X.astype(np.float64)[:, None, :] - X.astype(np.float64)[nn]) ** 2).sum(axis=2)
    assert np.allclose(d2, exact, rtol=1e-5, atol=0.0)


@pytest.mark.parametrize("dim", DIM_SET)
@pytest.mark.parametrize("n,K", [(n, K) for n in N_SET for K in (64, 65, 127, 128, 129, 255) if K <= n - 1])
def test_knn_passes_on_a_lattice(n, K, dim):
    """K > 63 on small-integer coordinates: every f32 distance is exact and ties abound, also across the pass edges 64 | 65,
    128 | 129 and 192 | 193 (asserted).  nn is numpy's lexsort by (d2, index), d2 is exact."""
    X = ref.lattice(n, dim, LATTICE_SIDE[dim], seed=n + K + dim)
    want_nn, want_d2 = ref.knn_lexsort(X, K)
    for edge in (64, 128, 192):
        if edge < K:
            assert (want_d2[:, edge - 1] == want_d2[:, edge]).any(), "no tie straddles entry %d | %d" % (edge, edge + 1)
    nn, d2 = knn(X, K)
    assert np.array_equal(d2, want_d2)
    assert np.array_equal(nn, want_nn)


def test_knn_copies_of_one_point():
    """Seventy copies (K = 69: the second pass starts inside the ties), seven copies (K = 6) and five copies among twenty
    other points: every copy lists the other copies in ascending index order at distance 0."""
    for n, K in ((70, 69), (7, 6)):
        nn, d2 = knn(np.full((n, 4), 2.5, dtype=np.float32), K)
        assert not d2.any()
        assert np.array_equal(nn, np.array([np.delete(np.arange(n), i) for i in range(n)]))
    X = np.random.default_rng(5).normal(size=(25, 3)).astype(np.float32) + 10.0
    copies = np.array([3, 8, 9, 17, 24])
    X[copies] = X[3]
    nn, d2 = knn(X, 6)
    for i in copies:
        assert np.array_equal(nn[i, :4], copies[copies != i]) and not d2[i, :4].any() and (d2[i, 4:] > 0).all()


# ---- T2, T3 ----------------------------------------------------------------------------------------------------------------------

def check_affinities(X, perplexity):
    g = tsne.affinities(X, perplexity)
    n, K = g.nn.shape
    beta, cond, _ = ref.calibrate(g.d2, perplexity)
    assert np.allclose(g.beta, beta, rtol=1e-9, atol=0.0)
    assert ulps(g.cond, cond.astype(np.float32)).max() <= 1
    rowptr, col, _, P32 = ref.joint(g.nn, cond)
    assert np.array_equal(g.rowptr, rowptr) and np.array_equal(g.col, col)
    assert ulps(g.P, P32).max() <= 1
    M = ref.dense(g.rowptr, g.col, g.P, np.float32)
    assert np.array_equal(M, M.T) and not M.diagonal().any()       # symmetric bit for bit, no diagonal
    assert abs(float(g.P.astype(np.float64).sum()) - 1.0) < 1e-6
    assert g.max_degree == int(np.diff(rowptr).max())
    return g


@pytest.mark.parametrize("perplexity", [2.0, 10.0, 30.0, 70.0])
def test_calibration_and_joint_distribution(perplexity):
    X = np.random.default_rng(int(perplexity)).normal(size=(300, 5)).astype(np.float32)
    g = check_affinities(X, perplexity)
    H = ref.calibrate(g.d2, perplexity)[2]
    assert np.allclose(np.exp(H), perplexity, rtol=1e-9)


def test_hub_row_crosses_the_wavefront():
    X = np.zeros((129, 64), dtype=np.float32)
    others = np.delete(np.arange(129), 64)                        # the hub sits in the middle of the index range
    X[others[:64], np.arange(64)] = 1.5
    X[others[64:], np.arange(64)] = -1.5
    g = check_affinities(X, 2.0)
    assert np.all(g.nn[others, 0] == 64)
    assert np.diff(g.rowptr)[64] == 128 and g.max_degree == 128


def test_duplicate_rows_stay_uniform():
    X = np.random.default_rng(8).normal(size=(40, 3)).astype(np.float32)
    X[10:20] = X[10]                                               # ten copies, K = 6: their rows are K duplicates
    g = check_affinities(X, 2.0)
    assert not g.d2[10:20].any()
    assert (g.beta[10:20] == 2.0 ** 100).all() and (g.cond[10:20] == np.float32(1.0 / 6.0)).all()


# ---- T4 ------------------------------------------------------------------------------------------------------------------------

def device_run(case, **kw):
    rowptr, col, P = tc.graph(case[0])
    args = dict(n_iter=tc.T8, learning_rate=tc.eta(case), early_exaggeration=tc.EXAG, exaggeration_iters=tc.EXAG_ITERS,
                momentum=tc.MOMENTUM, momentum_switch_iter=tc.SWITCH_ITER)
    args.update(kw)
    init = args.pop("init", None)
    init = tc.start(len(rowptr) - 1, case[1], case[2]) if init is None else init
    return tsne.layout(rowptr, col, P, init, **args)


@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_small_step(case):
    """T = 8 with both switches inside the run: G in {16, 32, 64} x c in {2, 3} x the starts 1e-4 normal and 4 normal, both
    sides of the G thresholds (mean row length 16, 16 + 1/n, 32, 32 + 1/n), every S(n) in {1, 2, 4, 8, 16} at both sides of
    its thresholds (n = 127 ... 1024), n = 2; every graph but that one has an empty row, which still moves (by repulsion: it
    is compared with the reference like any other), and a row longer than its lane group.  Observed on an MI355X (per case in
    the table of DESIGN.md section 5d): D32 5.35e-12 ... 2.31e-06, the device's error equal to D32 in all 34 cases, largest
    move 1.32e-06 ... 0.663, at least 21 400 D32."""
    rowptr, col, P, Y0, y64, d32, moved = tc.reference(case)
    n = len(rowptr) - 1
    Y = device_run(case)
    dev = float(np.abs(Y - y64).max())
    print("small step %s: D32 = %.3e, device = %.3e (%.2f D32), moved = %.3e" % (tc.case_id(case), d32, dev, dev / d32, moved))
    assert Y.dtype == np.float32 and Y.shape == (n, case[1])
    assert d32 > 0.0 and moved >= 1000.0 * d32
    assert dev <= 4.0 * d32
    empty = np.diff(rowptr) == 0
    if empty.any():
        centred = Y0 - Y0.mean(axis=0)
        assert np.abs(y64[empty] - centred[empty]).max() >= 1000.0 * d32       # the reference moves it ...
        assert np.abs(Y[empty] - y64[empty]).max() <= 4.0 * d32                 # ... and the device with it


@pytest.mark.parametrize("case", tc.ONE_STEP, ids=tc.case_id)
def test_one_iteration_from_a_chosen_state(case):
    """(Y, U, gains) after five fp64 iterations of the reference, then T = 1 at t0 = 5: gains_out exactly (but where the
    gradient's sign is rounding: |g64| < 4 |g32 - g64|, at most 1 % of the components, asserted on the reference alone in
    tests/test_tsne_host.py), U_out and Y_out to 4 D32 of their own.  Observed on an MI355X: no component left out in any case, Y at
    D32(Y) in all 32 cases, U at most 1.16 D32(U)."""
    Y, U, gains, y64, u64, want, unsure, d32y, d32u = tc.one_step(case)
    assert unsure.mean() <= 0.01
    Yd, (Ud, Gd), Z = device_run(case, init=Y, n_iter=1, first_iter=5, state=(U, gains), return_state=True, center=False)
    dy, du = float(np.abs(Yd - y64).max()), float(np.abs(Ud - u64).max())
    print("one step %s: D32(Y) = %.3e, device = %.3e; D32(U) = %.3e, device = %.3e; %d of %d gains left out"
          % (tc.case_id(case), d32y, dy, d32u, du, unsure.sum(), unsure.size))
    assert np.array_equal(Gd[~unsure], want[~unsure])
    assert dy <= 4.0 * d32y and du <= 4.0 * d32u
    rowptr, col, P = tc.graph(case[0])
    Zref = ref.gradient(ref.dense(rowptr, col, P), Y.astype(np.float64), 1.0)[1]
    # Z: fp64 over f32 chunk sums of at most 128 terms in (0, 1], each q one f32 step off: (128 + 1) 2^-24 < 1e-5 at the worst
    assert abs(Z - Zref) <= 1e-5 * Zref


@pytest.mark.parametrize("case", [("g16", 2, 4.0), ("g64", 3, 1e-4), ("n1023", 2, 4.0)], ids=tc.case_id)
def test_resume(case):
    """T = 8 in one call equals 3 (center off) + 5 (t0 = 3, the state passed on), bit for bit: coordinates, velocity, gains
    and the last normaliser.  The split straddles the exaggeration switch's side (t = 3) and the momentum switch (t = 5)."""
    whole = device_run(case, return_state=True)
    Y3, state3, _ = device_run(case, n_iter=3, return_state=True, center=False)
    rest = device_run(case, init=Y3, n_iter=5, first_iter=3, state=state3, return_state=True)
    assert np.array_equal(whole[0], rest[0])
    assert np.array_equal(whole[1][0], rest[1][0]) and np.array_equal(whole[1][1], rest[1][1]) and whole[2] == rest[2]
    # centring at the boundary is another trajectory in f32: the flag is not a no-op
    Y3c = device_run(case, n_iter=3, center=True)
    assert not np.array_equal(Y3c, Y3)
    assert np.abs(Y3c.astype(np.float64).mean(axis=0)).max() <= 1e-6 * np.abs(Y3).max()


def test_layout_refuses_a_vanishing_normaliser():
    """Two points 2e30 apart: |y_0 - y_1|^2 overflows f32, q rounds to 0 and Z = 0.  The call reports it (MI_EINVAL) instead
    of returning the NaN coordinates the division by Z left."""
    from scrna_seq_qannealing_clustering_amd import _lib
    rowptr, col, P = tc.graph("n2")
    Y0 = np.array([[1e30, 0.0], [-1e30, 0.0]], dtype=np.float32)
    with pytest.raises(_lib.MiSaError, match="normaliser Z") as ei:
        tsne.layout(rowptr, col, P, Y0, n_iter=2)
    assert ei.value.code == -1


# ---- the whole chain ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def blobs_run():
    X, labels = ref.blobs(seed=2, n=300, dim=10, sep=50.0)
    r = tsne.run_tsne(X, perplexity=10, n_iter=300, exaggeration_iters=100)
    return X, labels, r


def test_determinism(blobs_run):
    X, _, r = blobs_run
    again = tsne.run_tsne(X, perplexity=10, n_iter=300, exaggeration_iters=100)
    assert np.array_equal(r.coords, again.coords) and r.kl_divergence == again.kl_divergence
    g = r.graph
    assert tsne.kl_divergence(g.rowptr, g.col, g.P, r.coords) == tsne.kl_divergence(g.rowptr, g.col, g.P, r.coords) \
        == r.kl_divergence


def test_end_to_end_on_blobs(blobs_run):
    """Three planted blobs 50 standard deviations apart, n = 300, dim 10, perplexity 10, 300 iterations (exaggeration for
    100): every point's nearest neighbour in the picture carries its label; the KL divergence fell from its value at the
    start and is the reference's formula on the device's coordinates at rtol 1e-6 (f32 q on ~10^4 terms summed in fp64);
    the column means are zero to f32 rounding.  Observed on an MI355X: KL 3.174663 -> 0.966001666, the reference's formula
    0.966001670: a relative difference of 4.4e-9, 230 times inside the bound."""
    X, labels, r = blobs_run
    Y, g = r.coords, r.graph
    assert Y.dtype == np.float32 and Y.shape == (300, 2) and np.isfinite(Y).all()
    d = ((Y.astype(np.float64)[:, None, :] - Y.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    assert (labels[d.argmin(axis=1)] == labels).all()
    kl0 = tsne.kl_divergence(g.rowptr, g.col, g.P, tsne.random_init(300, 2, 1))
    want = ref.kl(g.rowptr, g.col, g.P, Y)
    print("KL: start %.6f, end %.9f, reference formula %.9f (rel %.2e)" % (kl0, r.kl_divergence, want,
                                                                          abs(r.kl_divergence - want) / want))
    assert r.kl_divergence < kl0
    assert abs(r.kl_divergence - want) <= 1e-6 * abs(want)
    assert np.abs(Y.astype(np.float64).mean(axis=0)).max() <= 2.0 ** -23 * np.abs(Y).max()
    assert set(r.timing) >= {"knn_ms", "calibrate_ms", "symmetrize_ms", "layout_ms", "iter_ms", "kl_ms", "total_ms"}


def test_run_tsne_is_affinities_then_layout():
    X = np.random.default_rng(11).normal(size=(101, 5)).astype(np.float32)
    for c, init in ((2, "random"), (3, "pca")):
        r = tsne.run_tsne(X, perplexity=5, n_components=c, n_iter=20, learning_rate=50.0, init=init, seed=7)
        g = tsne.affinities(X, 5)
        Y0 = tsne.random_init(101, c, 7) if init == "random" else tsne.scaled_pca_init(X, c)
        assert np.array_equal(r.graph.P, g.P) and np.array_equal(r.graph.col, g.col)
        assert np.array_equal(r.coords, tsne.layout(g.rowptr, g.col, g.P, Y0, 20, 50.0))
        for kw in (dict(n_iter=21), dict(learning_rate=60.0), dict(early_exaggeration=4.0), dict(exaggeration_iters=10),
                   dict(momentum=(0.4, 0.8)), dict(momentum_switch_iter=10)):
            args = dict(n_iter=20, learning_rate=50.0)
            args.update(kw)
            assert not np.array_equal(r.coords, tsne.layout(g.rowptr, g.col, g.P, Y0, **args)), kw
