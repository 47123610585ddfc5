"""Chain Q (mapping new points) without a GPU: the numpy restatement (tests/mapping_reference.py) against
umap_reference where the two overlap, the small-step criterion of tests/test_gpu_mapping.py shown to see every deliberate
deviation on every one of its cases, the vote on handmade rows, and every argument error of the library and of the Python
layer, each raised before any device work.  (MI_ESTATE needs an open handle: tests/test_gpu_mapping.py.)"""
import ctypes as C

import numpy as np
import pytest

import mapping_cases as mc
import mapping_reference as mref
import umap_reference as ref
from scrna_seq_qannealing_clustering_amd import _lib, mapping, umap

MI_EINVAL, MI_EUNSUPPORTED = -1, -5


# ---- 1. the restatement against umap_reference ------------------------------------------------------------------------------

def test_cross_knn_of_a_set_against_itself_is_knn_exact():
    X = np.random.default_rng(0).normal(size=(150, 6)).astype(np.float32)
    assert len(np.unique(X, axis=0)) == 150
    for k in (2, 9, 64):
        nn = mref.cross_knn(X, X, k)
        assert np.array_equal(nn, ref.knn_exact(X, k)) and np.array_equal(nn[:, 0], np.arange(150))
        assert np.array_equal(mref.distances(X, X, nn, "euclidean"), ref.distances(X, nn, "euclidean"))
        U = ref.normalize_rows(X)
        assert np.array_equal(mref.distances(U, U, nn, "cosine"), ref.distances(U, nn, "cosine"))


def test_smooth_normalises_to_log2_k_with_rho_zero():
    rng = np.random.default_rng(1)
    R, Q = rng.normal(size=(200, 6)).astype(np.float32), rng.normal(size=(40, 6)).astype(np.float32)
    for k in (2, 5, 15, 64):
        nn = mref.cross_knn(Q, R, k)
        dist = mref.distances(Q, R, nn, "euclidean")
        sigma, w, binds = mref.smooth(dist)
        assert not binds.any() and (np.diff(dist, axis=1) >= 0).all()
        v = np.exp(-dist.astype(np.float64) / sigma[:, None])
        assert np.abs(v.sum(axis=1) - np.log2(k)).max() < 1e-9 and np.array_equal(w, v.astype(np.float32))
        # a row does not depend on its batch
        s1, w1, _ = mref.smooth(dist[7:8])
        assert s1[0] == sigma[7] and np.array_equal(w1[0], w[7])
    # all distances 0: every weight exactly 1; zeros beyond log2(k) of them: sigma collapses and the floor binds
    sigma, w, binds = mref.smooth(np.array([[0, 0, 0, 0, 0], [0, 0, 0, 1, 2]], dtype=np.float32))
    assert np.array_equal(w[0], np.ones(5, dtype=np.float32)) and not binds[0]
    assert binds[1] and sigma[1] == 1e-3 * (3.0 / 5.0) and np.array_equal(w[1, :3], np.ones(3, dtype=np.float32)) and not w[1, 3:].any()
    y0 = mref.init(np.array([[0, 1, 2, 3, 4]]), w[:1], np.arange(10, dtype=np.float32).reshape(5, 2))
    assert np.array_equal(y0, [[4.0, 5.0]])                                   # the plain mean


def test_ratios_are_per_row():
    w = np.array([[0.5, 0.25, 0.0], [0.3, 0.1, 0.3]], dtype=np.float32)
    p = mref.ratios(w)
    assert p.dtype == np.float32 and np.array_equal(p[0], [1.0, 0.5, 0.0]) and p[1, 0] == 1.0 == p[1, 2]
    assert np.array_equal(p[1], mref.ratios(w[1:])[0]) and mref.ratios(w, "batch_max")[1, 0] == np.float32(0.3) / np.float32(0.5)


# ---- 2. the small-step criterion sees every deviation ---------------------------------------------------------------------

NEEDS_NEG = ("philox_t_q", "no_q0", "mod_m", "neg_from_queries", "keep_skip")


@pytest.mark.parametrize("G", [16, 32, 64])
def test_small_step_criterion_sees_errors(G):
    """For every case of tests/test_gpu_mapping.py: D32 is positive, the largest move is >= 1000 D32 (observed: >= 4332), and the
    float32 restatement with any one line of mref.MUTATIONS wrong lies more than the 4 D32 the device is allowed from y64.
    A deviation of the negatives cannot act without negatives, nor an ignored q0 at q0 = 0: those are skipped, everything else
    is asserted.  Smallest observed (distance / D32) where the deviation acts: philox_t_q 1842, no_q0 2917, mod_m 2197,
    neg_from_queries 7520, keep_skip 74, batch_max 1258, fire_next 1219, alpha_next 1083."""
    seen = {}
    for case in mc.CASES:
        k, c, neg, seed, q0, shape = case
        if mc.lanes(k) != G:
            continue
        nn, w, Yref, Y0, y64, d32, moved = mc.reference(case)
        assert d32 > 0.0 and moved >= 1000.0 * d32, mc.case_id(case)
        for m in mref.MUTATIONS:
            if (neg == 0 and m in NEEDS_NEG) or (q0 == 0 and m == "no_q0"):
                continue
            ym = mref.layout(nn, w, Yref, Y0, *mc.AB, mc.ALPHA0, mc.T8, neg, seed, q0, np.float32, mutate=m)
            away = float(np.abs(ym - y64).max())
            assert away > 4.0 * d32, (m, mc.case_id(case), away / d32)
            seen[m] = min(seen.get(m, np.inf), away / d32)
    assert set(seen) == set(mref.MUTATIONS), sorted(set(mref.MUTATIONS) - set(seen))


def test_handmade_rows_hold_what_they_claim():
    for T in (8, 10000):
        nn, w, Yref, Y0, facts = mc.handmade(T)
        fires = [ref.fire_counts(p, T) for p in facts["ratios"]]
        assert fires == [T, T - 1, int(np.floor(np.float32(T) * np.float32(1.0 / 3.0))), int(np.floor(np.float32(T) * np.float32(2.0 / 3.0))),
                         1, T // 2, T // 4, 0]
        assert w[1, 7] == 0.0 and (w.max(axis=1) == 0.5).all()
        hit = facts["hit"]
        assert nn[2, 0] == hit and np.array_equal(Y0[2], Yref[hit]) and mref.draws(2, 0, 0, 1, 8, 42)[0] == hit
        # the coincident start takes the +4 rule at epoch 0 and no attraction: one epoch, that entry alone
        y = mref.layout(nn[2:3, :1], w[2:3, :1], Yref, Y0[2:3], *mc.AB, mc.ALPHA0, 1, 1, 42, 2, np.float64)
        assert np.array_equal(y[0], Y0[2].astype(np.float64) + np.float64(np.float32(mc.ALPHA0)) * 4.0)
    with pytest.raises(AssertionError):
        mref.layout(nn, w, Yref, Y0, *mc.AB, mc.ALPHA0, 1, 1, 42, mutate="no such line")


# ---- 4. the vote ---------------------------------------------------------------------------------------------------------------

def test_vote_on_handmade_rows():
    labels = np.array([0, 0, 1, 1, 2, -1, -1, 4], dtype=np.int32)               # label 3 occurs nowhere
    nn = np.array([[2, 0, 3, 1], [5, 6, 5, 6], [4, 5, 0, 6], [7, 2, 3, 5]], dtype=np.int32)
    w = np.array([[0.5, 0.25, 0.25, 0.5], [1, 1, 1, 1], [0.25, 1, 0.75, 1], [0.5, 0.125, 0.125, 1]], dtype=np.float32)
    label, score, scores = mref.vote(nn, w, labels, 5)
    # row 0: labels 1 and 0 both weigh 0.75: the tie goes to the smaller; row 1: nobody is labelled; row 2: 0.75 beats 0.25,
    # the unlabelled neighbours' weight is not in the total; row 3: label 4 with 0.5 of 0.75
    assert label.tolist() == [0, -1, 0, 4] and score.tolist() == [0.5, 0.0, 0.75, 0.5 / 0.75]
    assert scores[0].tolist() == [0.5, 0.5, 0, 0, 0] and not scores[1].any() and scores[2].tolist() == [0.75, 0, 0.25, 0, 0]
    assert not scores[:, 3].any() and scores.shape == (4, 5)
    label, score, _ = mref.vote(nn, np.ones_like(w), labels, 5)
    assert label.tolist() == [0, -1, 0, 1] and score.tolist() == [0.5, 0.0, 0.5, 2.0 / 3.0]
    # a labelled neighbourhood whose weights are all 0 counts as unlabelled
    assert mref.vote(nn[:1], np.zeros((1, 4)), labels, 5)[0].tolist() == [-1]


# ---- 3. argument errors, each before device work --------------------------------------------------------------------------------

def library_error(name, *args):
    with pytest.raises(_lib.MiSaError) as ei:
        _lib.call(name, *args)
    return ei.value.code


def layout_args(**kw):
    f32 = np.float32
    a = dict(m=2, k=3, nn=np.array([[0, 1, 2], [3, 2, 1]], dtype=np.int32), w=np.array([[1, 0.5, 0], [0.2, 0.2, 0.1]], dtype=f32),
             n=4, c=2, Yref=np.zeros((4, 2), dtype=f32), Y0=np.zeros((2, 2), dtype=f32), a=1.0, b=1.0, alpha0=0.25, T=5, neg=5,
             seed=C.c_uint64(42), q0=C.c_int64(0), device=0, out=np.zeros((2, 2), dtype=f32), ms=None)
    a.update(kw)
    return list(a.values())


def test_library_argument_errors():
    """every one is MI_EINVAL or MI_EUNSUPPORTED, not MI_ENODEV: the check comes before the device is looked for (this runs
    where there is none)"""
    f32 = np.float32
    bad = [dict(nn=None), dict(w=None), dict(Yref=None), dict(Y0=None), dict(out=None), dict(m=0), dict(n=0), dict(k=0), dict(k=65),
           dict(nn=np.array([[0, 1, 4], [3, 2, 1]], dtype=np.int32)), dict(nn=np.array([[0, -1, 2], [3, 2, 1]], dtype=np.int32)),
           dict(w=np.array([[1, 0.5, 0], [0, 0, 0]], dtype=f32)),                  # a row whose largest weight is 0
           dict(w=np.array([[1, -0.5, 0], [1, 1, 1]], dtype=f32)), dict(w=np.array([[1, np.inf, 0], [1, 1, 1]], dtype=f32)),
           dict(w=np.array([[1, np.nan, 0], [1, 1, 1]], dtype=f32)), dict(T=0), dict(T=10001), dict(neg=-1), dict(neg=17),
           dict(a=np.inf), dict(b=np.nan), dict(alpha0=np.inf), dict(Yref=np.full((4, 2), np.nan, dtype=f32)),
           dict(Y0=np.full((2, 2), np.inf, dtype=f32)), dict(q0=C.c_int64(-1)), dict(q0=C.c_int64(2 ** 31 - 2))]
    for kw in bad:
        assert library_error("mi_umap_transform_layout_f32", *layout_args(**kw)) == MI_EINVAL, kw
    assert library_error("mi_umap_transform_layout_f32", *layout_args(c=4)) == MI_EUNSUPPORTED
    assert library_error("mi_umap_transform_layout_f32", *layout_args(c=1)) == MI_EUNSUPPORTED
    assert library_error("mi_umap_transform_layout_f32", *layout_args(n=(1 << 23) + 1)) == MI_EUNSUPPORTED
    R, Q, h = np.zeros((5, 2), dtype=f32), np.ones((3, 2), dtype=f32), C.c_void_p()
    knn = dict(R=R, n=5, Q=Q, m=3, dim=2, k=3, metric=0, device=0, out=h, ms=None)
    wide = np.zeros((5, 2), dtype=f32)
    wide[0, 0], wide[1, 0] = -3e38, 3e38                                          # a squared distance would overflow
    for kw in (dict(R=None), dict(Q=None), dict(out=None), dict(n=1), dict(m=0), dict(dim=0), dict(dim=65), dict(k=1), dict(k=6),
               dict(k=65), dict(metric=2), dict(R=np.full((5, 2), np.nan, dtype=f32)), dict(Q=np.full((3, 2), np.inf, dtype=f32)),
               dict(R=wide), dict(R=wide / 2, Q=np.full((3, 2), -3e38, dtype=f32))):  # ... the range over R and Q together
        args = dict(knn)
        args.update(kw)
        assert library_error("mi_umap_query_knn_f32", *args.values()) == MI_EINVAL, kw
    assert library_error("mi_umap_query_knn_f32", *dict(knn, n=(1 << 23) + 1).values()) == MI_EUNSUPPORTED
    assert h.value is None
    assert library_error("mi_umap_query_fetch_knn", None, None, None) == MI_EINVAL
    assert library_error("mi_umap_query_smooth", None, None) == MI_EINVAL
    assert library_error("mi_umap_query_fetch_smooth", None, None, None) == MI_EINVAL
    assert library_error("mi_umap_query_vote", None, np.zeros(5, dtype=np.int32), 1, 0, np.zeros(3, dtype=np.int32), np.zeros(3), None,
                         None) == MI_EINVAL
    assert library_error("mi_umap_query_init", None, 2, np.zeros((5, 2), dtype=f32), np.zeros((3, 2), dtype=f32), None) == MI_EINVAL
    assert _lib.call("mi_umap_query_destroy", None) == 0


def test_python_argument_errors(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("an argument error must be raised before the library is touched")
    monkeypatch.setattr(_lib, "load", no_library)
    rng = np.random.default_rng(4)
    R, Q = rng.normal(size=(20, 4)).astype(np.float32), rng.normal(size=(7, 4)).astype(np.float32)
    lab = np.arange(20) % 3
    model = umap.UmapResult(coords=np.zeros((20, 2), dtype=np.float32), a=1.0, b=1.0, n_epochs=30)
    bad_points = [dict(X_new=Q[0]), dict(X_new=Q[:0]), dict(X_new=Q[:, :3]), dict(X_new=Q.astype(str)),
                  dict(X_new=np.where(np.arange(28).reshape(7, 4) == 5, np.nan, Q)), dict(X_ref=R[:1]), dict(X_ref=R[0]),
                  dict(X_ref=np.where(np.arange(80).reshape(20, 4) == 5, np.inf, R)), dict(k=1), dict(k=21), dict(k=2.5),
                  dict(k=65, X_ref=np.zeros((70, 4))), dict(metric="manhattan"),
                  dict(X_new=np.zeros((7, 65)), X_ref=np.zeros((20, 65)))]
    for kw in bad_points:
        args = dict(X_new=Q, X_ref=R, k=5, metric="euclidean")
        args.update(kw)
        with pytest.raises(ValueError):
            mapping.cross_knn(**args)
        with pytest.raises(ValueError):
            mapping.transfer_labels(args["X_new"], args["X_ref"], lab[:len(args["X_ref"])], args["k"], args["metric"])
        with pytest.raises(ValueError):
            umap.transform(args["X_new"], args["X_ref"], model, n_neighbors=args["k"], metric=args["metric"])
    for kw in (dict(labels_ref=lab[:19]), dict(labels_ref=lab.astype(float)), dict(labels_ref=np.full(20, -1)),
               dict(labels_ref=lab.reshape(4, 5)), dict(weights="gaussian")):
        args = dict(X_new=Q, X_ref=R, labels_ref=lab, k=5)
        args.update(kw)
        with pytest.raises(ValueError):
            mapping.transfer_labels(**args)
    X = np.concatenate([R, Q])
    for kw in (dict(kept=np.arange(20.0)), dict(kept=np.array([0])), dict(kept=np.array([0, 0, 1])), dict(kept=np.array([0, 27])),
               dict(kept=np.array([-1, 3])), dict(labels_kept=lab[:19]), dict(labels_kept=lab.astype(float)), dict(X=X[0]),
               dict(return_scores=True), dict(k=1)):
        args = dict(X=X, kept=np.arange(20), labels_kept=lab)
        args.update(kw)
        with pytest.raises(ValueError):
            mapping.extend_labels(**args)

    class NoEpochs:
        coords, a, b = model.coords, 1.0, 1.0
    for kw in (dict(model=NoEpochs()), dict(model=umap.UmapResult(model, coords=np.zeros((19, 2)))),
               dict(model=umap.UmapResult(model, coords=np.zeros((20, 4)))), dict(model=umap.UmapResult(model, a=np.nan)),
               dict(model=umap.UmapResult(model, coords=np.full((20, 2), np.inf))), dict(model=umap.UmapResult(model, n_epochs=0)),
               dict(n_epochs=0), dict(n_epochs=10001), dict(n_epochs=1.5), dict(learning_rate=0.0), dict(negative_sample_rate=17),
               dict(seed=-1), dict(first_index=-1), dict(first_index=2 ** 31 - 7), dict(first_index=0.5)):
        args = dict(X_new=Q, X_ref=R, model=model, n_neighbors=5)
        args.update(kw)
        with pytest.raises(ValueError):
            umap.transform(**args)
    nn, w = np.array([[0, 1], [2, 3]]), np.array([[1.0, 0.5], [0.5, 0.0]])
    for kw in (dict(nn=nn.astype(float)), dict(nn=nn[0]), dict(nn=np.zeros((2, 65), dtype=int), w=np.ones((2, 65))),
               dict(nn=np.array([[0, 1], [2, 4]])), dict(nn=np.array([[0, -1], [2, 3]])), dict(w=w[:1]),
               dict(w=np.array([[1.0, 0.5], [0.0, 0.0]])), dict(w=np.array([[1.0, -0.5], [0.5, 0.0]])),
               dict(w=np.array([[1.0, np.nan], [0.5, 0.0]])), dict(Yref=np.zeros((4, 4))), dict(Yref=np.full((4, 2), np.inf)),
               dict(init=np.zeros((2, 3))), dict(init=np.full((2, 2), np.nan)), dict(a=np.inf), dict(alpha0=0.0), dict(n_epochs=0),
               dict(negative_sample_rate=-1), dict(seed=2 ** 64), dict(first_index=-1), dict(first_index=2 ** 31 - 2)):
        args = dict(nn=nn, w=w, Yref=np.zeros((4, 2)), init=np.zeros((2, 2)), a=1.0, b=1.0, alpha0=0.25, n_epochs=5)
        args.update(kw)
        with pytest.raises(ValueError):
            umap.transform_layout(**args)


def test_a_closed_query_graph_refuses_before_the_library(monkeypatch):
    g = mapping.QueryGraph.__new__(mapping.QueryGraph)
    g.n, g.m, g.k = 5, 3, 2
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was entered"))
    for use in (lambda: g.fetch_knn(), lambda: g.smooth(), lambda: g.fetch_smooth(), lambda: g.vote(np.zeros(5, dtype=np.int32), 1),
                lambda: g.init(np.zeros((5, 2)))):
        with pytest.raises(ValueError, match="the QueryGraph is closed"):
            use()


def test_the_package_exports_the_module():
    import scrna_seq_qannealing_clustering_amd as pkg
    assert pkg.mapping is mapping and "mapping" in pkg.__all__
    assert umap.transform.__defaults__[:2] == (30, "cosine")
    assert {"mi_umap_query_knn_f32", "mi_umap_query_destroy", "mi_umap_query_fetch_knn", "mi_umap_query_smooth",
            "mi_umap_query_fetch_smooth", "mi_umap_query_vote", "mi_umap_query_init", "mi_umap_transform_layout_f32"} <= set(_lib.EXPORTS)
