"""Chain A on the CPU: the numpy restatement (tests/anchor_reference.py) has the chain's properties on
the cases of tests/anchor_cases.py, the cases plant what they claim and are sharp where tests/test_gpu_anchors.py compares
labels, and the Python layer's argument checks come before any call into the library.  No device."""
import ctypes as C
import math

import numpy as np
import pytest

import anchor_cases as ac
import anchor_reference as aref
from scrna_seq_qannealing_clustering_amd import _lib, anchors


@pytest.mark.parametrize("name", ac.SMALL)
def test_anchors_are_mutual_bounded_and_ordered(name):
    c, f = ac.case(name), ac.found(name)
    ka, ks = c["kw"]["k_anchor"], c["kw"]["k_score"]
    pairs, raw = f["pairs"], f["raw"]
    assert len(pairs) >= 1
    for r, q in pairs:
        assert q in f["RQ"][r, :ka] and r in f["QR"][q, :ka]
    assert np.bincount(pairs[:, 0]).max() <= ka and np.bincount(pairs[:, 1]).max() <= ka
    rank = np.array([int(np.flatnonzero(f["RQ"][r, :ka] == q)[0]) for r, q in pairs])
    key = pairs[:, 0].astype(np.int64) * 64 + rank
    assert (np.diff(key) > 0).all()                               # ascending r, then q's rank in RQ[r]
    assert raw.min() >= 0 and raw.max() <= 2 * ks
    assert (f["score"] >= 0).all() and (f["score"] <= 1).all()
    assert np.array_equal(f["RR"][:, 0], np.arange(len(c["Xr"]))) or name in ("dk0",)        # a cell is its own first neighbour
    assert np.array_equal(f["U"], np.unique(pairs[:, 1]))


@pytest.mark.parametrize("name", [n for n in ac.SMALL if n not in ("copy", "dk0", "tie", "equal_raw")])
def test_cases_avoid_exact_distance_ties(name):
    """the order of a kNN row is then the distances' alone (the cases left out tie on purpose: the index decides)"""
    f = ac.found(name)
    import mapping_reference as mref
    for A, B, T in ((f["R"], f["R"], f["RR"]), (f["R"], f["Q"], f["RQ"]), (f["Q"], f["R"], f["QR"]), (f["Q"], f["Q"], f["QQ"])):
        d2 = mref.chain_d2(A, B, np.broadcast_to(np.arange(len(B)), (len(A), len(B))))
        d2 = np.sort(d2, axis=1)[:, :T.shape[1] + 1]
        assert (np.diff(d2, axis=1) > 0).all()


def test_planted_structure():
    f = ac.found("copy")
    ks = ac.case("copy")["kw"]["k_score"]
    own = f["pairs"][:, 0] == f["pairs"][:, 1]
    assert own.sum() == 60 and (f["raw"][own] == 2 * ks).all() and f["raw"].min() < 2 * ks
    f = ac.found("hole")
    per_ref = np.bincount(f["pairs"][:, 0], minlength=80)
    assert per_ref[40] == 0 and per_ref[0] > 0 and per_ref[79] > 0
    f = ac.found("dk0")
    assert f["U"].tolist() == [0, 1, 2, 3, 4]
    w = ac.weighted("dk0", 5)
    assert not w["WD"][:30].any() and (w["WD"][30:, 0] == w["WD"][30:, 4]).all() and (w["WD"][30:] > 0).all()
    sums = aref.row_sums(w["rowptr"], w["weight"])
    assert (sums[:30] > 0).all() and not sums[30:].any()          # dk = 0 rows carry weight, the others are zero rows
    f = ac.found("equal_raw")
    assert len(set(f["raw"].tolist())) == 1 and (f["score"] == 1.0).all()
    f = ac.found("kmin")
    assert ac.case("kmin")["kw"]["k_score"] == len(ac.case("kmin")["Xq"]) == f["QQ"].shape[1]
    assert ac.case("ka_eq_ks")["kw"]["k_anchor"] == ac.case("ka_eq_ks")["kw"]["k_score"]
    for name, kw, _ in ac.WEIGHT_CASES:
        assert (kw or 2) <= ac.n_anchor_queries(name)
    assert ac.n_anchor_queries("blobs4") >= 64
    assert {1, 64} <= {ac.case(n)["Xr"].shape[1] for n in ac.SMALL}


@pytest.mark.parametrize("name, k_weight, sd", ac.WEIGHT_CASES, ids=lambda v: str(v))
def test_weight_rows_sum_to_one(name, k_weight, sd):
    """Every entry is its weight over the row's total, rounded once: the EXACT sum of a non-zero row (math.fsum, so that the
    check adds no rounding of its own) lies within 4 ulp of 1.  Rows are at most k_weight * k_anchor long."""
    name, kw, sd = ac.weight_case(name, k_weight, sd)
    w, ka = ac.weighted(name, kw, sd), ac.case(name)["kw"]["k_anchor"]
    rowptr, weight = w["rowptr"], w["weight"]
    assert np.diff(rowptr).max() <= kw * ka and (weight >= 0).all()
    nonzero = 0
    for c in range(len(rowptr) - 1):
        row = weight[rowptr[c]:rowptr[c + 1]]
        if row.any():
            nonzero += 1
            assert abs(math.fsum(row) - 1.0) <= 4 * np.spacing(1.0)
    assert nonzero >= 1


def test_planted_labels_are_recovered_on_separated_blobs():
    c, f, w = ac.case("blobs4"), ac.found("blobs4"), ac.weighted("blobs4", 50)
    label, score, scores = aref.predict_labels(w["rowptr"], w["anchor"], w["weight"], f["pairs"], c["blob_ref"].astype(np.int32), 4)
    assert (label == c["blob_query"]).mean() >= 0.95
    np.testing.assert_allclose(scores.sum(axis=1), 1.0, rtol=1e-12)
    assert np.array_equal(score, scores.max(axis=1))


def test_label_cases_are_sharp():
    """the share of query cells whose two best class scores lie within 1e-9 is at most 1 % wherever labels are compared"""
    from scrna_seq_qannealing_clustering_amd.mapping import _check_labels
    f, w = ac.found("blobs4"), ac.weighted("blobs4", 50)
    for name, labels in ac.label_sets().items():
        codes, classes = _check_labels(labels, 300)
        _, _, scores = aref.predict_labels(w["rowptr"], w["anchor"], w["weight"], f["pairs"], codes, len(classes))
        assert aref.near_ties(scores).mean() <= 0.01, name
    sets = ac.label_sets()
    assert (sets["planted"] < 0).sum() == 60 and set(sets["odd_values"].tolist()) == {7, -3, 1000}
    assert len(set(sets["one_class"].tolist())) == 1 and len(set(sets["own_class"].tolist())) == 300
    c, f = ac.case("subsample"), ac.found("subsample")
    w = ac.weighted("subsample", 50)
    _, _, scores = aref.predict_labels(w["rowptr"], w["anchor"], w["weight"], f["pairs"], c["blob_ref"].astype(np.int32), 6)
    assert aref.near_ties(scores).mean() <= 0.01


def test_tie_case_ties_exactly():
    """two classes, mirror-image anchors: both class sums are the same additions of the same numbers"""
    c, f = ac.case("tie"), ac.found("tie")
    assert np.array_equal(f["pairs"], np.stack([np.arange(12), np.repeat(np.arange(6), 2)], axis=1))
    assert (f["raw"][0::2] == f["raw"][1::2]).all()
    w = ac.weighted("tie", c["k_weight"])
    codes = (c["labels"] == 11).astype(np.int32)                  # classes sorted: 4 -> 0, 11 -> 1
    label, score, scores = aref.predict_labels(w["rowptr"], w["anchor"], w["weight"], f["pairs"], codes, 2)
    assert (scores[:, 0] == scores[:, 1]).all() and (scores[:, 0] > 0).all() and not label.any()


def test_constant_feature_and_zero_rows():
    f, w = ac.found("dk0"), ac.weighted("dk0", 5)
    ref = np.full((20, 3), 4.0, dtype=np.float32)
    pred = aref.predict_features(w["rowptr"], w["anchor"], w["weight"], f["pairs"], ref)
    sums = aref.row_sums(w["rowptr"], w["weight"])
    assert (pred == 4.0 * sums[:, None]).all() and not pred[30:].any()            # (a power of two: every product is exact)
    f, w = ac.found("blobs4"), ac.weighted("blobs4", 50)
    pred = aref.predict_features(w["rowptr"], w["anchor"], w["weight"], f["pairs"], np.full((300, 1), 0.5, dtype=np.float32))[:, 0]
    sums = aref.row_sums(w["rowptr"], w["weight"])
    assert (pred == 0.5 * sums).all() and (sums == 1.0).sum() >= 10 and (pred[sums == 1.0] == 0.5).all()


# ---- argument checks: all raised before any call into the library --------------------------------------------------------------

@pytest.fixture
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "call", refuse)
    monkeypatch.setattr(_lib, "call_ms", refuse)
    monkeypatch.setattr(_lib, "load", refuse)


def test_point_set_checks(no_library):
    rng = np.random.default_rng(0)
    R, Q = rng.normal(size=(40, 5)).astype(np.float32), rng.normal(size=(30, 5)).astype(np.float32)
    with pytest.raises(ValueError, match="dim = 5"):
        anchors.find_transfer_anchors(Q[:, :4], R)
    with pytest.raises(ValueError, match="1 <= dim <= 64"):
        anchors.find_transfer_anchors(np.zeros((30, 65)), np.ones((40, 65)))
    with pytest.raises(ValueError, match="numeric"):
        anchors.find_transfer_anchors(Q[0], R)
    with pytest.raises(ValueError, match=r"min\(n, m, 64\)"):
        anchors.find_transfer_anchors(Q, R, k_score=31)                       # K = 31 > m = 30
    with pytest.raises(ValueError, match=r"min\(n, m, 64\)"):
        anchors.find_transfer_anchors(Q, R[:20], k_score=21)                  # K = 21 > n = 20
    with pytest.raises(ValueError, match=r"min\(n, m, 64\)"):
        anchors.find_transfer_anchors(np.tile(Q, (3, 1)), np.tile(R, (3, 1)), k_anchor=65)
    with pytest.raises(ValueError, match="k_anchor"):
        anchors.find_transfer_anchors(Q, R, k_anchor=1)
    with pytest.raises(ValueError, match="finite"):
        anchors.find_transfer_anchors(np.where(np.arange(5) == 2, np.nan, Q), R)
    Z = R.copy()
    Z[7] = 0.0
    with pytest.raises(ValueError, match="row 7 of X_ref is all zero"):
        anchors.find_transfer_anchors(Q, Z)
    with pytest.raises(ValueError, match="row 7 of X_query is all zero"):
        anchors.map_query(Z[:30], R, np.zeros(40, dtype=np.int64))
    with pytest.raises(ValueError, match="refdata"):
        anchors.map_query(Q, R, np.zeros(39, dtype=np.int64))


def test_refdata_and_weight_checks(no_library):
    with pytest.raises(ValueError, match=r"exceeds \|U\| = 17"):
        anchors._check_k_weight(18, 17)
    anchors._check_k_weight(17, 17)
    for bad in (1, 65, 2.5, True):
        with pytest.raises(ValueError, match="k_weight"):
            anchors._check_weight_args(bad, 1.0)
    for bad in (0.0, -1.0, float("inf"), float("nan"), "1"):
        with pytest.raises(ValueError, match="sd_weight"):
            anchors._check_weight_args(50, bad)
    ref = np.ones((4, 3), dtype=np.float32)
    with pytest.raises(ValueError, match="2\\^31"):
        anchors._check_refdata(ref, 4, (2 ** 31 + 2) // 3)                    # m * F >= 2^31
    assert anchors._check_refdata(ref, 4, (2 ** 31 - 1) // 3)[0] == "features"
    with pytest.raises(ValueError, match="finite"):
        anchors._check_refdata(ref * np.inf, 4, 10)
    with pytest.raises(ValueError, match="refdata must be"):
        anchors._check_refdata(np.ones(4), 4, 10)                             # a float vector is neither labels nor (n, F)
    with pytest.raises(ValueError, match="no label"):
        anchors._check_refdata(np.full(4, -1), 4, 10)
    kind, codes, classes = anchors._check_refdata(np.array([7, -3, 1000, 7]), 4, 10)
    assert kind == "labels" and codes.tolist() == [0, -1, 1, 0] and classes.tolist() == [7, 1000]
    with pytest.raises(ValueError, match="empty"):
        anchors._check_refdata_arg({}, 4, 10, False)


def test_transfer_checks_on_an_open_set_come_before_the_library(no_library):
    """an AnchorSet as find_transfer_anchors leaves it, without a device: k_weight > |U| and bad refdata are refused first"""
    aset = anchors.AnchorSet.__new__(anchors.AnchorSet)
    aset.n, aset.m, aset.n_anchor_queries, aset._weights_key, aset.timing = 40, 30, 17, None, {}
    aset._h = C.c_void_p(1)                                                   # (never dereferenced: no_library)
    try:
        with pytest.raises(ValueError, match=r"k_weight = 50 exceeds \|U\| = 17"):
            anchors.transfer_data(aset, np.zeros(40, dtype=np.int64))
        with pytest.raises(ValueError, match="refdata must be"):
            anchors.transfer_data(aset, np.zeros(41, dtype=np.int64), k_weight=10)
        with pytest.raises(ValueError, match="before weights"):
            aset.predict_features(np.ones((40, 2)))
    finally:
        aset._h = None
    with pytest.raises(ValueError, match="closed"):
        anchors.transfer_data(aset, np.zeros(40, dtype=np.int64))
    assert aset.device_bytes() == 0


def test_normalize_scores_is_the_restatements():
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 61, size=500).astype(np.int32)
    assert np.array_equal(anchors.normalize_scores(raw), aref.normalize_scores(raw))
    assert (anchors.normalize_scores(np.full(9, 12, dtype=np.int32)) == 1.0).all()
    s = anchors.normalize_scores(raw)
    assert s.min() == 0.0 and s.max() == 1.0
