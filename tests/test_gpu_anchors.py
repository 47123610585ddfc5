"""Chain A on the device (csrc/anchor_kernels.hip) against its numpy restatement
(tests/anchor_reference.py) on the cases of tests/anchor_cases.py: the anchor list, the raw scores and the four kNN tables
exactly; the weight CSR's structure exactly and its values at the project's RTOL for fp64 chains with a transcendental (the
sums run in one order on both sides, so only expm1 differs); class scores at RTOL and labels wherever the two best scores are
not within 1e-9 (tests/test_anchor_cases.py shows that to be at most 1 % of the cells); feature predictions within one f32
step; bit-identical repeats; and map_query against its parts."""
import numpy as np
import pytest

import anchor_cases as ac
import anchor_reference as aref
import mapping_reference as mref
from scrna_seq_qannealing_clustering_amd import anchors, umap
from scrna_seq_qannealing_clustering_amd.mapping import _check_labels

pytestmark = pytest.mark.gpu

RTOL = 1e-9


def open_case(name):
    c = ac.case(name)
    return anchors.find_transfer_anchors(c["Xq"], c["Xr"], **c["kw"])


def within_one_step(got, want64):
    """f32 `got` at most one f32 step from float32(want64)"""
    want = np.asarray(want64).astype(np.float32)
    return bool((np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.maximum(np.abs(got), np.abs(want)))).all())


# ---- 1, 2: pairs, raw scores, tables ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ac.SMALL)
def test_pairs_raw_scores_and_tables_exact(name):
    f = ac.found(name)
    with open_case(name) as a:
        tables = a.fetch_tables()
        assert a.anchors.dtype == np.int32 and np.array_equal(a.anchors, f["pairs"])
        assert a.raw_score.dtype == np.int32 and np.array_equal(a.raw_score, f["raw"])
        assert np.array_equal(a.score, f["score"]) and a.n_anchor_queries == len(f["U"])
        for got, key in zip(tables, ("RR", "RQ", "QR", "QQ")):
            assert got.dtype == np.int32 and np.array_equal(got, f[key]), key
        assert set(a.timing) >= {"knn_ms", "pairs_ms", "score_ms"}


def test_more_than_65536_anchors():
    """n = m = 20 000: the scan crosses its 1024-cell tile and the fills their first workgroups many times over.  The tables
    are checked on sampled rows (Q1 itself is tests/test_gpu_mapping.py's subject), then A2 and A3 of the restatement run on
    the device's tables."""
    c = ac.case("big")
    with open_case("big") as a:
        RR, RQ, QR, QQ = a.fetch_tables()
        pairs, raw = a.anchors, a.raw_score
    rows = np.random.default_rng(0).choice(20000, 64, replace=False)
    for T, A, B in ((RR, c["Xr"], c["Xr"]), (RQ, c["Xr"], c["Xq"]), (QR, c["Xq"], c["Xr"]), (QQ, c["Xq"], c["Xq"])):
        assert np.array_equal(T[rows], aref.cross_knn(A[rows], B, 5))
    want = aref.anchor_pairs(RQ, QR, 5)
    assert len(want) > 65536 and np.array_equal(pairs, want)
    assert np.array_equal(raw, aref.anchor_raw(want, RR, RQ, QR, QQ, 5))
    assert np.bincount(pairs[:, 0]).max() <= 5 and np.bincount(pairs[:, 1]).max() <= 5


# ---- 3: weights -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, k_weight, sd", ac.WEIGHT_CASES, ids=lambda v: str(v))
def test_weights(name, k_weight, sd):
    name, kw, sd = ac.weight_case(name, k_weight, sd)
    want = ac.weighted(name, kw, sd)
    with open_case(name) as a:
        got = a.weights(kw, sd)
        assert "weight_knn_ms" in a.timing and "weights_ms" in a.timing
    assert np.array_equal(got.wn, want["WN"]) and np.array_equal(got.wd, want["WD"])
    assert got.rowptr.dtype == np.int64 and np.array_equal(got.rowptr, want["rowptr"])
    assert got.anchor.dtype == np.int32 and np.array_equal(got.anchor, want["anchor"])
    np.testing.assert_allclose(got.weight, want["weight"], rtol=RTOL, atol=0.0)
    assert np.array_equal(got.weight == 0.0, want["weight"] == 0.0)
    if name == "dk0":
        sums = aref.row_sums(got.rowptr, got.weight)
        assert (sums[:30] > 0).all() and not sums[30:].any() and not got.wd[:30].any()


def test_k_weight_beyond_the_anchor_queries_is_refused():
    with open_case("kmin") as a:
        with pytest.raises(ValueError, match=r"exceeds \|U\| = %d" % a.n_anchor_queries):
            a.weights(a.n_anchor_queries + 1)
        a.weights(a.n_anchor_queries)


# ---- 4: labels ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["planted", "odd_values", "one_class", "own_class"])
def test_labels(which):
    labels_ref = ac.label_sets()[which]
    codes, classes = _check_labels(labels_ref, 300)
    f, w = ac.found("blobs4"), ac.weighted("blobs4", 50)
    want_label, want_score, want_scores = aref.predict_labels(w["rowptr"], w["anchor"], w["weight"], f["pairs"], codes, len(classes))
    with open_case("blobs4") as a:
        res = anchors.transfer_data(a, labels_ref, return_scores=True)
        plain = anchors.transfer_data(a, labels_ref)
    assert res.scores.shape == (200, len(classes)) and np.array_equal(res.classes, classes)
    np.testing.assert_allclose(res.scores, want_scores, rtol=RTOL, atol=0.0)
    np.testing.assert_allclose(res.score, want_score, rtol=RTOL, atol=0.0)
    sure = ~aref.near_ties(want_scores)
    assert sure.mean() >= 0.99
    want_values = np.where(want_label >= 0, classes[np.maximum(want_label, 0)], -1)
    assert np.array_equal(res.labels[sure], want_values[sure])
    assert set(res.labels.tolist()) <= set(classes.tolist()) | {-1}
    assert np.array_equal(plain.labels, res.labels) and np.array_equal(plain.score, res.score) and "scores" not in plain
    if which == "odd_values":
        assert set(res.labels.tolist()) <= {7, 1000, -1} and {7, 1000} <= set(res.labels.tolist())
    if which == "one_class":
        assert set(res.labels.tolist()) <= {5, -1} and (res.labels == 5).mean() > 0.9
    if which == "own_class":
        assert len(classes) == 300 and res.labels.max() >= 10 + 64               # a class beyond the first round of lanes wins


def test_exact_ties_go_to_the_smaller_label():
    c = ac.case("tie")
    with open_case("tie") as a:
        res = anchors.transfer_data(a, c["labels"], k_weight=c["k_weight"], return_scores=True)
    assert res.classes.tolist() == [4, 11]
    assert (res.scores[:, 0] == res.scores[:, 1]).all() and (res.scores > 0).all()
    assert (res.labels == 4).all() and np.array_equal(res.score, res.scores[:, 0])


def test_rows_without_weight_get_no_label():
    with open_case("dk0") as a:
        res = anchors.transfer_data(a, np.arange(20) % 3, k_weight=5, return_scores=True)
        pred = anchors.transfer_data(a, np.full((20, 65), 4.0, dtype=np.float32), k_weight=5).predicted
        sums = aref.row_sums(*[a.weights(5)[k] for k in ("rowptr", "weight")])
    assert (res.labels[:30] >= 0).all() and (res.labels[30:] == -1).all() and not res.score[30:].any() and not res.scores[30:].any()
    # a constant column of a power of two: every product is exact, the prediction is c * (row sum), and c where that is 1
    assert (pred == (4.0 * sums).astype(np.float32)[:, None]).all() and not pred[30:].any()
    assert (pred[sums == 1.0] == 4.0).all()


# ---- 5: features ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [1, 63, 64, 65, 228, 300])
def test_features(F):
    f, w = ac.found("blobs4"), ac.weighted("blobs4", 50)
    rng = np.random.default_rng(F)
    ref = rng.gamma(2.0, 2.0, size=(300, F)).astype(np.float32)              # protein-like: no cancellation within a row's sum
    ref[:, 0] = 0.5
    want = aref.predict_features(w["rowptr"], w["anchor"], w["weight"], f["pairs"], ref)
    with open_case("blobs4") as a:
        got = anchors.transfer_data(a, ref).predicted
        rows = a.weights(50)
    assert got.dtype == np.float32 and got.shape == (200, F)
    # against the restatement, and against its last stage on the device's own weights (the weights' 1e-9 is far below a step)
    assert within_one_step(got, want)
    assert within_one_step(got, aref.predict_features(rows.rowptr, rows.anchor, rows.weight, f["pairs"], ref))
    sums = aref.row_sums(rows.rowptr, rows.weight)
    # a constant column of a power of two: every product is exact, so the prediction is c * (row sum), and c where that is 1
    assert (got[:, 0] == (0.5 * sums).astype(np.float32)).all() and (sums == 1.0).sum() >= 10 and (got[sums == 1.0, 0] == 0.5).all()


# ---- 6: determinism ---------------------------------------------------------------------------------------------------------------

def test_two_calls_and_a_dict_return_the_same_bits():
    c = ac.case("blobs4")
    labels_ref = ac.label_sets()["planted"]
    adt = np.random.default_rng(1).normal(size=(300, 17)).astype(np.float32)
    runs = []
    for _ in range(2):
        with open_case("blobs4") as a:
            w = a.weights(50)
            lab = anchors.transfer_data(a, labels_ref, return_scores=True)
            feat = anchors.transfer_data(a, adt)
            both = anchors.transfer_data(a, {"celltype": labels_ref, "ADT": adt}, return_scores=True)
            runs.append((a.anchors, a.raw_score, a.score, *a.fetch_tables(), w.rowptr, w.anchor, w.weight, w.wn, w.wd,
                         lab.labels, lab.score, lab.scores, feat.predicted))
        assert set(both) == {"celltype", "ADT"}
        assert np.array_equal(both["celltype"].labels, lab.labels) and np.array_equal(both["celltype"].score, lab.score)
        assert np.array_equal(both["celltype"].scores, lab.scores) and np.array_equal(both["ADT"].predicted, feat.predicted)
    for x, y in zip(*runs):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert c["Xq"].flags.writeable is False


# ---- 7: map_query -----------------------------------------------------------------------------------------------------------------

def test_map_query_is_its_parts():
    c = ac.case("subsample")
    Xr, Xq, labels_ref = c["Xr"], c["Xq"], c["blob_ref"]
    assert Xr.shape == (1000, 15) and Xq.shape == (1638, 15)
    um = umap.run_umap(Xr, n_neighbors=15, n_epochs=30)
    kw = dict(n_neighbors=15, n_epochs=10)
    res = anchors.map_query(Xq, Xr, labels_ref, um=um, umap_kw=kw)
    with anchors.find_transfer_anchors(Xq, Xr) as a:
        start = a.device_bytes()
        assert start > 0
        direct = anchors.transfer_data(a, labels_ref)
        with_weights = a.device_bytes()
        anchors.transfer_data(a, {"l": labels_ref, "f": Xr[:, :3]})
        assert a.device_bytes() == with_weights > start                           # predictions leave nothing behind
        assert np.array_equal(res.anchors, a.anchors)
    assert a.device_bytes() == 0
    with pytest.raises(ValueError, match="closed"):
        a.weights()
    assert np.array_equal(res.transfer.labels, direct.labels) and np.array_equal(res.transfer.score, direct.score)
    assert (res.transfer.labels == c["blob_query"]).mean() >= 0.95
    placed = umap.transform(Xq, Xr, um, **kw)
    assert res.coords.dtype == np.float32 and np.array_equal(res.coords, placed.coords)
    assert "coords" not in anchors.map_query(Xq, Xr, labels_ref)
