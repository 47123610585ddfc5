"""Chain Q on the device (csrc/mapping_kernels.hip) against its numpy restatement
(tests/mapping_reference.py), each stage's restatement fed the device's previous-stage output: the cross kNN on integer
coordinates (exact distances, frequent ties) at every KM x DP instantiation, its distances on real-valued points, the smooth
weights and the weighted-mean start at the project's tolerances, k_umap_transform under the small-step criterion
|Y - y64| <= 4 D32 (which tests/test_mapping_host.py shows to see every deliberate deviation), independence of a query from its
batch bit for bit, the vote, and the sub-sample -> extend -> transform flow on planted blobs."""
import numpy as np
import pytest

import mapping_cases as mc
import mapping_reference as mref
import umap_reference as ref
from scrna_seq_qannealing_clustering_amd import _lib, mapping, umap

pytestmark = pytest.mark.gpu

RTOL = 1e-9


def ulps(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert (a >= 0).all() and (b >= 0).all()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def within_one_step(a, b):
    """signed f32 values at most one f32 step apart"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return bool((np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))).all())


# ---- Q1 ------------------------------------------------------------------------------------------------------------------------

# (m, n, k, dim): every KM bucket (k <= 8, 16, 32, 64; both edges of each) x every DP bucket (dim <= 16, 32, 64)
EXACT = [(1, 2, 2, 1), (63, 63, 8, 15), (65, 67, 8, 17), (130, 131, 2, 33),
         (1, 63, 9, 1), (63, 67, 9, 16), (65, 131, 16, 17), (130, 257, 16, 64),
         (65, 63, 17, 15), (130, 67, 32, 17), (63, 257, 32, 33), (130, 131, 17, 64),
         (130, 131, 33, 16), (1, 257, 64, 17), (65, 67, 64, 64), (63, 131, 33, 33)]
assert {((k > 8) + (k > 16) + (k > 32), (d > 16) + (d > 32)) for _, _, k, d in EXACT} == {(a, b) for a in range(4) for b in range(3)}
assert {k for _, _, k, _ in EXACT} == {2, 8, 9, 16, 17, 32, 33, 64} and {d for *_, d in EXACT} == {1, 15, 16, 17, 33, 64}
assert {m for m, *_ in EXACT} == {1, 63, 65, 130} and {n for _, n, _, _ in EXACT} == {2, 63, 67, 131, 257}
assert any(m > n for m, n, _, _ in EXACT) and any(m < n for m, n, _, _ in EXACT)


@pytest.mark.parametrize("m, n, k, dim", EXACT, ids=lambda v: str(v))
def test_cross_knn_exact_on_integer_points(m, n, k, dim):
    """Coordinates are integers in [-8, 8]: every f32 d2 is exact (<= 64 * 256), ties are frequent, and the order (d2, index) is
    the whole result.  A third of the reference rows are copies of other reference rows and half of the queries copies of
    reference rows: those find distance 0 at the lowest index that holds the row."""
    rng = np.random.default_rng(m * 1000 + n + k + dim)
    R = rng.integers(-8, 9, size=(n, dim)).astype(np.float32)
    dup = rng.choice(n, n // 3, replace=False)
    R[dup] = R[rng.integers(0, n, size=len(dup))]
    Q = rng.integers(-8, 9, size=(m, dim)).astype(np.float32)
    Q[::2] = R[rng.integers(0, n, size=len(Q[::2]))]
    nn, dist = mapping.cross_knn(Q, R, k)
    want = mref.cross_knn(Q, R, k)
    assert nn.dtype == np.int32 and nn.shape == (m, k) and np.array_equal(nn, want)
    assert ulps(dist, mref.distances(Q, R, want, "euclidean")).max() <= 2     # (exact d2: what is left is sqrtf)
    assert not dist[::2, 0].any()
    first = [int(np.flatnonzero((R == q).all(axis=1))[0]) for q in Q[::2]]
    assert nn[::2, 0].tolist() == first
    if n > 2:
        d2 = (dist.astype(np.float64) ** 2).round()
        assert (d2[:, 1:] == d2[:, :-1]).any() or k == 2                      # ties within the lists


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_cross_knn_on_real_points(metric):
    rng = np.random.default_rng(11)
    R, Q = rng.normal(size=(203, 15)).astype(np.float32), rng.normal(size=(77, 15)).astype(np.float32)
    Q[5] = 0.0                                                                # a zero query row: cosine leaves it zero
    nn, dist = mapping.cross_knn(Q, R, 30, metric)
    Qs, Rs = (ref.normalize_rows(Q), ref.normalize_rows(R)) if metric == "cosine" else (Q, R)
    assert ulps(dist, mref.distances(Qs, Rs, nn, metric)).max() <= 2
    assert np.isfinite(dist).all() and (np.diff(dist, axis=1) >= 0).all()
    exact = np.sort(((Qs[:, None, :].astype(np.float64) - Rs[None].astype(np.float64)) ** 2).sum(axis=2), axis=1)[:, :30]
    exact = exact / 2.0 if metric == "cosine" else np.sqrt(exact)
    np.testing.assert_allclose(dist, exact, rtol=1e-5, atol=1e-7)
    if metric == "cosine":
        np.testing.assert_allclose(dist[5], 0.5, rtol=1e-6)                   # |0 - u|^2 / 2
    # a set against itself is chain U1, column for column
    nn_self, dist_self = mapping.cross_knn(R, R, 30, metric)
    nn_u, dist_u = umap.knn(R, 30, metric)
    assert np.array_equal(nn_self, nn_u) and np.array_equal(dist_self, dist_u)


# ---- Q2, Q3 --------------------------------------------------------------------------------------------------------------------

def check_smooth_init(g, Yref):
    """Q2 and Q3 of an open QueryGraph against the restatement on the device's own distances / sigma / weights"""
    nn, dist = g.fetch_knn()
    sigma, w = g.smooth().fetch_smooth()
    want_sigma, _, binds = mref.smooth(dist)
    np.testing.assert_allclose(sigma, want_sigma, rtol=RTOL, atol=0.0)
    assert w.dtype == np.float32 and ulps(w, mref.weights(dist, sigma)).max() <= 1
    y0 = g.init(Yref)
    assert y0.dtype == np.float32 and within_one_step(y0, mref.init(nn, w, Yref))
    return nn, dist, sigma, w, y0, binds


@pytest.mark.parametrize("k, c, metric", [(2, 2, "euclidean"), (15, 3, "cosine"), (30, 2, "cosine"), (64, 3, "euclidean")])
def test_smooth_and_init(k, c, metric):
    rng = np.random.default_rng(k)
    R, Q = rng.normal(size=(300, 10)).astype(np.float32), rng.normal(size=(259, 10)).astype(np.float32)
    Yref = (rng.normal(size=(300, c)) * 5.0).astype(np.float32)
    with mapping.QueryGraph(Q, R, k, metric) as g:
        nn, dist, sigma, w, y0, binds = check_smooth_init(g, Yref)
    assert not binds.any() and (w.max(axis=1) < 1.0).all()
    v = np.exp(-dist.astype(np.float64) / sigma[:, None])
    assert np.abs(v.sum(axis=1) - np.log2(k)).max() < 1e-9


def test_smooth_special_rows():
    """Query 0 sits on five copies of one reference point with k = 5: all distances 0, every weight exactly 1, sigma = 2^-64
    (64 halvings; the floor is 0) and the start is the plain mean.  Query 1 sits on three copies of another (3 > log2 5 zeros:
    the bisection collapses) with two neighbours further out: the floor 1e-3 * (the row's mean distance) binds."""
    rng = np.random.default_rng(5)
    R = rng.normal(size=(40, 4)).astype(np.float32) + 10.0
    R[:5] = [1.0, 2.0, 3.0, 4.0]
    R[5:8] = [-3.0, 0.0, 1.0, 0.5]
    Q = np.concatenate([R[:1], R[5:6], rng.normal(size=(3, 4)).astype(np.float32) + 10.0])
    Yref = (rng.normal(size=(40, 2)) * 5.0).astype(np.float32)
    with mapping.QueryGraph(Q, R, 5) as g:
        nn, dist, sigma, w, y0, binds = check_smooth_init(g, Yref)
    assert nn[0].tolist() == [0, 1, 2, 3, 4] and not dist[0].any() and np.array_equal(w[0], np.ones(5, dtype=np.float32))
    assert sigma[0] == 2.0 ** -64
    mean = np.zeros(2)
    for p in range(5):
        mean = mean + Yref[p].astype(np.float64)
    assert np.array_equal(y0[0], (mean / 5.0).astype(np.float32))
    assert binds.tolist() == [False, True, False, False, False] and nn[1, :3].tolist() == [5, 6, 7]
    assert sigma[1] == 1e-3 * ((float(dist[1, 3]) + float(dist[1, 4])) / 5.0)
    assert np.array_equal(w[1, :3], np.ones(3, dtype=np.float32)) and not w[1, 3:].any()


# ---- Q4 ------------------------------------------------------------------------------------------------------------------------

def small_step(nn, w, Yref, Y0, T, neg, seed, q0, label):
    y64 = mref.layout(nn, w, Yref, Y0, *mc.AB, mc.ALPHA0, T, neg, seed, q0, np.float64)
    y32 = mref.layout(nn, w, Yref, Y0, *mc.AB, mc.ALPHA0, T, neg, seed, q0, np.float32)
    Y = umap.transform_layout(nn, w, Yref, Y0, *mc.AB, mc.ALPHA0, T, neg, seed, q0)
    d32, dev, moved = float(np.abs(y32 - y64).max()), float(np.abs(Y - y64).max()), float(np.abs(y64 - Y0).max())
    print("small step %s: D32 = %.3e, device = %.3e, moved = %.3e" % (label, d32, dev, moved))
    assert Y.dtype == np.float32 and Y.shape == Y0.shape
    assert d32 > 0.0 and moved >= 1000.0 * d32
    assert dev <= 4.0 * d32
    return Y


@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_small_step_every_instantiation(case):
    """k in {5, 16, 17, 32, 33, 64} (G = 16, 16, 32, 32, 64, 64: every group width, both sides of each threshold) x c in {2, 3} x
    neg in {0, 1, 5, 16}; seed 42 and one with a non-zero high word, q0 in {0, 1000}, (m, n) = (37, 67) and (83, 67): m is no
    multiple of the 256 / G queries of a workgroup."""
    k, c, neg, seed, q0, shape = case
    nn, w, Yref, Y0, y64, d32, moved = mc.reference(case)
    Y = umap.transform_layout(nn, w, Yref, Y0, *mc.AB, mc.ALPHA0, mc.T8, neg, seed, q0)
    dev = float(np.abs(Y - y64).max())
    print("small step %s: D32 = %.3e, device = %.3e, moved = %.3e" % (mc.case_id(case), d32, dev, moved))
    assert Y.dtype == np.float32 and Y.shape == (mc.SHAPES[shape][0], c)
    assert d32 > 0.0 and moved >= 1000.0 * d32
    assert dev <= 4.0 * d32


@pytest.mark.parametrize("T, c", [(8, 2), (8, 3), (10000, 2)])
def test_small_step_handmade_rows(T, c):
    """mc.handmade: ratios 1, one step below 1, 1/3, 2/3, 1/T, 1/2, 1/4 and one step below 1/T; a stored weight of 0; a start on
    a reference position that is also that entry's first negative of epoch 0 (no attraction at s = 0, then the +4 rule).
    T = 8 and T = MI_UMAP_MAX_EPOCHS.  An entry that never fires can be given the weight 0 without changing a bit."""
    assert umap.MAX_EPOCHS == 10000
    nn, w, Yref, Y0, facts = mc.handmade(T, c)
    Y = small_step(nn, w, Yref, Y0, T, 1, 42, 0, "handmade T = %d, c = %d" % (T, c))
    w0 = w.copy()
    w0[0, 7] = 0.0
    assert ref.fire_counts(facts["ratios"][7], T) == 0
    assert np.array_equal(Y, umap.transform_layout(nn, w0, Yref, Y0, *mc.AB, mc.ALPHA0, T, 1, 42, 0))


@pytest.mark.parametrize("c", [2, 3])
def test_small_step_500_epochs(c):
    nn, w, Yref, Y0 = mc.rows(16, c, "m<n")
    small_step(nn, w, Yref, Y0, 500, 5, 42, 1000, "T = 500, c = %d" % c)


# ---- independence and determinism, bit for bit -------------------------------------------------------------------------------

def test_a_query_does_not_depend_on_its_batch():
    rng = np.random.default_rng(21)
    R, Q = rng.normal(size=(150, 8)).astype(np.float32), rng.normal(size=(90, 8)).astype(np.float32)
    lab = rng.integers(0, 4, size=150)
    fit = umap.run_umap(R, n_neighbors=15, metric="euclidean", n_epochs=30, seed=3)
    kw = dict(n_neighbors=15, metric="euclidean", n_epochs=20, seed=9)
    t = umap.transform(Q, R, fit, **kw)
    again = umap.transform(Q, R, fit, **kw)
    assert t.n_epochs == 20 and umap.transform(Q[:2], R, fit, n_neighbors=15, metric="euclidean").n_epochs == 10
    for key in ("coords", "init", "nn", "dist", "sigma", "weights"):
        assert np.array_equal(t[key], again[key]), key
    assert not np.array_equal(t.coords, t.init) and np.isfinite(t.coords).all()
    a, b = 17, 60
    part = umap.transform(Q[a:b], R, fit, first_index=a, **kw)
    assert np.array_equal(part.coords, t.coords[a:b]) and np.array_equal(part.sigma, t.sigma[a:b])
    assert not np.array_equal(umap.transform(Q[a:b], R, fit, **kw).coords, t.coords[a:b])      # ... and first_index is why
    # every other row replaced (far larger distances: another batch maximum, another mean): row i is unchanged
    i = 41
    Q2 = (rng.normal(size=Q.shape) * 30.0).astype(np.float32)
    Q2[i] = Q[i]
    t2 = umap.transform(Q2, R, fit, **kw)
    for key in ("coords", "sigma", "weights", "nn", "dist", "init"):
        assert np.array_equal(t2[key][i], t[key][i]), key
    l1 = mapping.transfer_labels(Q, R, lab, k=15, return_scores=True)
    l2 = mapping.transfer_labels(Q2, R, lab, k=15, return_scores=True)
    assert l1.labels[i] == l2.labels[i] and l1.score[i] == l2.score[i] and np.array_equal(l1.scores[i], l2.scores[i])


# ---- Q5 ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weights", ["fuzzy", "uniform"])
def test_vote_against_the_restatement(weights):
    """L = 70 classes (no multiple of 64; k = 8 neighbours see at most 8 of them), a third of the reference unlabelled, and a
    far cluster of reference points without any label: the queries near it get -1."""
    rng = np.random.default_rng(31)
    R = rng.normal(size=(331, 5)).astype(np.float32)
    R[300:] += 50.0
    Q = rng.normal(size=(141, 5)).astype(np.float32)
    Q[130:] += 50.0
    codes = rng.integers(0, 70, size=331).astype(np.int32)
    codes[rng.random(331) < 0.33] = -1
    codes[300:] = -1
    codes[codes == 69] = 68
    codes[codes == 13] = 12                                                   # classes no query can see, the last one among them
    with mapping.QueryGraph(Q, R, 8) as g:
        nn, _ = g.fetch_knn()
        if weights == "fuzzy":
            with pytest.raises(_lib.MiSaError) as ei:                         # MI_ESTATE: the weights do not exist yet
                g.vote(codes, 70, "fuzzy")
            assert ei.value.code == -6
            u = g.smooth().fetch_smooth()[1]
        else:
            u = np.ones(nn.shape)
        label, score, scores = g.vote(codes, 70, weights, return_scores=True)
        l2, s2 = g.vote(codes, 70, weights)
    wl, ws, wd = mref.vote(nn, u, codes, 70)
    assert np.array_equal(label, wl) and np.array_equal(l2, wl) and np.array_equal(s2, score)
    np.testing.assert_allclose(score, ws, rtol=RTOL, atol=0.0)
    np.testing.assert_allclose(scores, wd, rtol=RTOL, atol=0.0)
    assert scores.shape == (141, 70) and np.array_equal(scores == 0.0, wd == 0.0) and not scores[:, [13, 69]].any()
    assert (label[130:] == -1).all() and not score[130:].any() and not scores[130:].any() and (label[:130] >= 0).all()
    if weights == "uniform":                                                  # ties: the smaller label won
        top = np.sort(wd[:130], axis=1)[:, -2:]
        tied = np.flatnonzero(top[:, 0] == top[:, 1])
        assert len(tied) >= 10
        assert all(label[i] == np.flatnonzero(wd[i] == wd[i].max())[0] for i in tied)


def test_transfer_labels_returns_the_callers_values():
    rng = np.random.default_rng(32)
    R, Q = rng.normal(size=(60, 3)).astype(np.float32), rng.normal(size=(25, 3)).astype(np.float32)
    values = np.array([-7, 40, 3, 1000])[rng.integers(0, 4, size=60)]         # -7: unlabelled
    res = mapping.transfer_labels(Q, R, values, k=6, weights="uniform", return_scores=True)
    assert res.classes.tolist() == [3, 40, 1000] and set(res.labels.tolist()) <= {3, 40, 1000, -1}
    codes = np.searchsorted(res.classes, np.where(values >= 0, values, 3)).astype(np.int32)
    codes[values < 0] = -1
    wl, ws, wd = mref.vote(res.nn, np.ones(res.nn.shape), codes, 3)
    assert np.array_equal(res.labels, np.where(wl >= 0, res.classes[np.maximum(wl, 0)], -1))
    np.testing.assert_allclose(res.scores, wd, rtol=RTOL, atol=0.0)
    assert "knn_ms" in res.timing and "vote_ms" in res.timing and "smooth_ms" not in res.timing


# ---- end to end ----------------------------------------------------------------------------------------------------------------

def test_sub_sample_extend_transform_on_blobs():
    """Three blobs, 399 kept / 201 held out: label transfer and extend_labels return the planted label of every held-out
    point, and after run_umap on the kept points and transform of the others, every held-out point's nearest kept point in the
    embedding carries its label."""
    X, planted = ref.blobs(seed=0, n=600, dim=10, sep=10.0)
    held = np.sort(np.random.default_rng(1).permutation(600)[:201])
    kept = np.setdiff1d(np.arange(600), held)
    assert len(kept) == 399 and set(planted[held]) == set(planted[kept]) == {0, 1, 2}
    for weights in ("fuzzy", "uniform"):
        res = mapping.transfer_labels(X[held], X[kept], planted[kept], k=15, weights=weights)
        assert np.array_equal(res.labels, planted[held]) and (res.score == 1.0).all()
    ext = mapping.extend_labels(X, kept, planted[kept], k=15)
    assert np.array_equal(ext.labels, planted) and np.array_equal(ext.held_out, held) and (ext.score == 1.0).all()
    fit = umap.run_umap(X[kept], n_neighbors=15, metric="euclidean")
    t = umap.transform(X[held], X[kept], fit, n_neighbors=15, metric="euclidean")
    assert t.n_epochs == fit.n_epochs // 3 == 166 and t.coords.shape == (201, 2)
    d2 = ((t.coords[:, None, :].astype(np.float64) - fit.coords[None].astype(np.float64)) ** 2).sum(axis=2)
    assert np.array_equal(planted[kept][d2.argmin(axis=1)], planted[held])
    assert set(t.timing) >= {"knn_ms", "smooth_ms", "init_ms", "layout_ms", "host_ms", "total_ms"}


# ---- the handle ----------------------------------------------------------------------------------------------------------------

def test_query_graph_lifetime_and_call_order():
    R, Q = np.array([[0.0], [1.0]], dtype=np.float32), np.array([[0.25]], dtype=np.float32)
    g = mapping.QueryGraph(Q, R, 2)
    assert g._handle().value and g.fetch_knn()[0].tolist() == [[0, 1]]
    for early in (lambda: g.fetch_smooth(), lambda: g.init(np.zeros((2, 2))), lambda: g.vote(np.zeros(2, dtype=np.int32), 1, "fuzzy")):
        with pytest.raises(_lib.MiSaError) as ei:
            early()
        assert ei.value.code == -6                                            # MI_ESTATE
    assert g.vote(np.zeros(2, dtype=np.int32), 1, "uniform")[0].tolist() == [0]
    g.close()
    g.close()
    assert g._h is None
    with pytest.raises(ValueError, match="the QueryGraph is closed"):
        g.fetch_knn()
    with mapping.QueryGraph(Q, R, 2) as again:
        assert again.smooth().fetch_smooth()[1].shape == (1, 2)
    with pytest.raises(ValueError, match="the QueryGraph is closed"):
        again._handle()
