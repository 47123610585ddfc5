"""Marker-gene detection, the parts that need no GPU: the closed forms of ``metrics.markers_from_stats`` on the CPU
reference's sufficient statistics (tests/markers_reference.py) against ``scipy.stats.mannwhitneyu``, the degenerate
statistics, Seurat's filter and ``top_markers`` on a hand-made example, and the argument validation of
``mi_rank_sum_markers_f32``, which happens before any device work."""
import ctypes as C

import numpy as np
import pytest
from scipy.stats import mannwhitneyu

from markers_reference import reference_stats, sparse_matrix
from scrna_seq_qannealing_clustering_amd import _lib, metrics

EINVAL, EUNSUPPORTED = -1, -5
P_RTOL = 1e-12


def columns(rng, n, g):
    """sparse, integer-tied and Gaussian columns, interleaved"""
    X = sparse_matrix(rng, n, g)
    X[:, 1::3] = rng.integers(0, 4, (n, len(range(1, g, 3))))
    X[:, 2::3] = rng.standard_normal((n, len(range(2, g, 3))))
    return X


@pytest.mark.parametrize("n,g,K", [(65, 7, 3), (257, 9, 4), (1000, 5, 9)])
def test_closed_forms_against_scipy(n, g, K):
    rng = np.random.default_rng(n)
    X = columns(rng, n, g)
    lab = rng.integers(0, K, n)
    lab[:K] = np.arange(K)
    rank2, npos, sums, tie, sizes = reference_stats(X, lab[None], K)
    r = metrics.markers_from_stats(rank2[0], npos[0], sums[0], tie, sizes[0], n)
    for j in range(g):
        for c in range(K):
            a, b = X[lab == c, j], X[lab != c, j]
            want = mannwhitneyu(a, b, use_continuity=True, method="asymptotic")
            assert r["U"][j, c] == want.statistic
            assert abs(r["p_val"][j, c] - want.pvalue) <= P_RTOL * want.pvalue
            assert r["auc"][j, c] == want.statistic / (len(a) * len(b))
            assert r["pct_1"][j, c] == (a > 0).mean() and r["pct_2"][j, c] == (b > 0).mean()
            m1, m2 = np.expm1(a.astype(np.float64)).mean(), np.expm1(b.astype(np.float64)).mean()
            assert abs(r["avg_log2FC"][j, c] - (np.log2(m1 + 1) - np.log2(m2 + 1))) <= 1e-9
    assert np.array_equal(r["p_val_adj"], np.minimum(1.0, r["p_val"] * g))


def test_degenerate_statistics():
    rng = np.random.default_rng(1)
    n = 40
    X = sparse_matrix(rng, n, 3)
    X[:, 1] = 2.5                                                   # a constant gene: sigma = 0
    lab = rng.integers(0, 2, n) * 2                                 # label 1 is empty
    rank2, npos, sums, tie, sizes = reference_stats(X, lab[None], 3)
    r = metrics.markers_from_stats(rank2[0], npos[0], sums[0], tie, sizes[0], n)
    assert np.isnan(r["p_val"][1]).all() and np.isnan(r["p_val_adj"][1]).all()
    assert np.isnan(r["p_val"][:, 1]).all() and np.isnan(r["auc"][:, 1]).all() and np.isnan(r["pct_1"][:, 1]).all()
    assert np.isfinite(r["p_val"][[0, 2]][:, [0, 2]]).all()
    assert (r["p_val_adj"][[0, 2]][:, [0, 2]] <= 1.0).all()
    assert np.any(r["p_val"] * 3 > 1.0)                             # ... so the clip at 1 did something
    # K = 1: there are no other cells
    rank2, npos, sums, tie, sizes = reference_stats(X, np.zeros((1, n), dtype=int), 1)
    r = metrics.markers_from_stats(rank2[0], npos[0], sums[0], tie, sizes[0], n)
    for key in ("p_val", "p_val_adj", "auc", "pct_2", "avg_log2FC"):
        assert np.isnan(r[key]).all(), key
    assert not metrics.markers_passed(r).any()
    # a leading labelling axis broadcasts
    L = rng.integers(0, 3, (4, n))
    st = reference_stats(X, L, 3)
    many = metrics.markers_from_stats(*st, n)
    for b in range(4):
        one = metrics.markers_from_stats(st[0][b], st[1][b], st[2][b], st[3], st[4][b], n)
        for key in one:
            assert np.array_equal(many[key][b], one[key], equal_nan=True), key


def six_cells():
    """6 cells, clusters 7 = {0, 1, 2} and 9 = {3, 4, 5}; genes a .. e"""
    X = np.array([[1, 0, 2, 0, 0.0],
                  [1, 0, 2, 0, 0.0],
                  [1, 0, 3, 0, 0.5],
                  [0, 1, 1, 0, 0.0],
                  [0, 1, 1, 0, 0.0],
                  [0, 1, 1, 0, 0.0]], dtype=np.float32)
    return X, np.array([7, 7, 7, 9, 9, 9]), np.array(list("abcde"))


def test_filter_and_top_markers_by_hand():
    X, lab, genes = six_cells()
    K, n = 2, 6
    rank2, npos, sums, tie, sizes = reference_stats(X, (lab == 9)[None].astype(int), K)
    r = metrics.markers_from_stats(rank2[0], npos[0], sums[0], tie, sizes[0], n)
    # gene a: the three 1s hold the ranks 4, 5, 6 (midrank 5), the zeros 1, 2, 3 (midrank 2)
    assert rank2[0, 0].tolist() == [30, 12] and tie[0] == 48 and r["U"][0].tolist() == [9.0, 0.0]
    assert r["pct_1"][:, 0].tolist() == [1.0, 0.0, 1.0, 0.0, 1 / 3] and r["pct_2"][:, 0].tolist() == [0.0, 1.0, 1.0, 0.0, 0.0]
    e = np.expm1(1.0)
    assert abs(r["avg_log2FC"][0, 0] - np.log2(e + 1)) < 1e-12 and abs(r["avg_log2FC"][0, 1] + np.log2(e + 1)) < 1e-12
    assert np.isnan(r["p_val"][3]).all()                            # gene d is constant
    pos = metrics.markers_passed(r, only_pos=True, min_pct=0.25, logfc_threshold=0)
    # only_pos keeps a, c, e for cluster 7 and b for cluster 9; d passes the fold-change test at threshold 0 but not min_pct
    assert pos.T.tolist() == [[True, False, True, False, True], [False, True, False, False, False]]
    both = metrics.markers_passed(r, only_pos=False, min_pct=0.25, logfc_threshold=0.25)
    assert both.T.tolist() == [[True, True, True, False, True], [True, True, True, False, True]]
    assert not metrics.markers_passed(r, min_pct=0.34)[4].any()      # round(1 / 3, 3) = 0.333 < 0.34
    assert metrics.markers_passed(r, min_pct=0.333)[4].all()
    res = dict(r, passed=pos, cluster_ids=np.array([7, 9]), genes=genes)
    fc = r["avg_log2FC"][:, 0]
    assert fc[2] > fc[0] > fc[4] > 0
    assert metrics.top_markers(res, n=2) == {7: ["c", "a"], 9: ["b"]}
    assert metrics.top_markers(res, n=5) == {7: ["c", "a", "e"], 9: ["b"]}
    tied = dict(res, avg_log2FC=np.where(pos, 1.0, r["avg_log2FC"]))
    assert metrics.top_markers(tied, n=2) == {7: ["a", "c"], 9: ["b"]}      # ties: gene order
    with pytest.raises(ValueError):
        metrics.top_markers(res, labelling=1)


def call(X, n, g, L, B, K, flags=0, rank2="alloc"):
    f32p, u16p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_uint16), C.POINTER(C.c_int64)
    out = np.zeros(max(B * g * K, 1), dtype=np.int64) if rank2 == "alloc" else None
    return _lib.load().mi_rank_sum_markers_f32(
        None if X is None else X.ctypes.data_as(f32p), n, g, None if L is None else L.ctypes.data_as(u16p), B, K, 0, flags,
        None if out is None else out.ctypes.data_as(i64p), None, None, None, None)


def test_argument_validation_needs_no_device():
    lib = _lib.load()
    n, g, B, K = 5, 3, 2, 4
    X = np.ones((n, g), dtype=np.float32)
    L = np.zeros((B, n), dtype=np.uint16)
    assert call(None, n, g, L, B, K) == EINVAL and b"NULL" in lib.mi_last_error()
    assert call(X, n, g, None, B, K) == EINVAL
    assert call(X, n, g, L, B, K, rank2=None) == EINVAL
    assert call(X, 0, g, L, B, K) == EINVAL and call(X, n, 0, L, B, K) == EINVAL and call(X, n, g, L, 0, K) == EINVAL
    assert call(X, n, g, L, B, 0) == EINVAL
    assert call(X, n, g, L, B, 65) == EINVAL and b"K" in lib.mi_last_error()
    assert call(X, n, g, L, B, K, flags=4) == EINVAL and b"flags" in lib.mi_last_error()
    bad = L.copy()
    bad[1, 3] = K
    assert call(X, n, g, bad, B, K) == EINVAL and b"label" in lib.mi_last_error()
    for v in (np.nan, np.inf, -np.inf):
        Xb = X.copy()
        Xb[4, 2] = v
        assert call(Xb, n, g, L, B, K) == EINVAL and b"finite" in lib.mi_last_error()
    big = (1 << 20) + 1
    assert call(np.zeros((big, 1), dtype=np.float32), big, 1, np.zeros((1, big), dtype=np.uint16), 1, 1) == EUNSUPPORTED
    # B * g * K above the cap (2^28 entries), refused before X (far smaller than n x g here) is read
    assert call(X, n, 1 << 23, L, B, 64) == EUNSUPPORTED
    with pytest.raises(_lib.MiSaError) as ei:
        metrics.rank_sum_pass(X, bad, K)
    assert ei.value.code == EINVAL
    with pytest.raises(ValueError):
        metrics.rank_sum_pass(X, np.zeros((B, n + 1), dtype=int), K)
    with pytest.raises(ValueError):
        metrics.find_all_markers(X, np.arange(n * 13).reshape(13, n))             # 65 distinct ids


def test_constants_match_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mi_metrics.h")).read()
    val = lambda name: int(re.search(r"#define %s\s+(\d+)" % name, hdr).group(1))
    assert metrics.MARKERS_LDS_MAX_NONZEROS == val("MI_MARKERS_LDS_MAX_NONZEROS") >= 8192
    assert metrics.MARKERS_LABELLING_CHUNK == val("MI_MARKERS_LABELLING_CHUNK")
