"""Pins oracle/metrics_oracle.py: the Jaccard distance matrix against scipy's, the silhouette widths against
scikit-learn's independent implementation, a hand-computed 4-point case, and the float64-product pair counts
against the int64 product and against popcounts of the packed bit rows.  CPU only.  (The R packages
the reference calls -- proxy, cluster, fpc -- are absent; see the oracle's header.)"""
import numpy as np
import pytest
from scipy.spatial.distance import pdist, squareform
from sklearn.metrics import silhouette_samples

from oracle import metrics_oracle as mo


def test_distance_and_silhouette_against_independent_implementations():
    rng = np.random.RandomState(0)
    X = (rng.rand(200, 300) < 0.15) * rng.rand(200, 300)
    lab = rng.randint(0, 5, size=200)
    D = mo.jaccard_distance_matrix(X)
    assert np.allclose(D, squareform(pdist(X != 0, "jaccard")), rtol=0, atol=1e-15)
    assert np.allclose(mo.silhouette_widths(D, lab), silhouette_samples(D, lab, metric="precomputed"), rtol=0, atol=1e-15)


def test_hand_computed_case():
    # genes: A={0,1}, B={0,1}, C={2,3}, D={2}  -> d(A,B)=0, d(C,D)=1/2, every cross distance 1
    X = np.array([[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 1, 1], [0, 0, 1, 0]])
    st = mo.cluster_stats(mo.jaccard_distance_matrix(X), np.array([0, 0, 1, 1]))
    assert st["diameter"].tolist() == [0.0, 0.5] and st["separation"].tolist() == [1.0, 1.0]
    assert st["average.between"] == 1.0 and st["average.within"] == 0.25 and st["dunn"] == 2.0
    assert st["n.within"] == 2 and st["n.between"] == 4
    assert np.allclose(st["sil.widths"], [1.0, 1.0, 0.5, 0.5])
    assert st["within.cluster.ss"] == 0.125


def _pattern(n, g, seed):
    rng = np.random.RandomState(seed)
    X = (rng.rand(n, g) < 0.15) * rng.rand(n, g)
    X[n // 3] = 0                                                # empty rows: union 0 with each other
    X[n // 2] = 0
    return X


@pytest.mark.parametrize("n,g", [(1, 1), (7, 63), (40, 64), (33, 65), (120, 500), (300, 3001)])
def test_pair_counts_distances_equal_the_int64_product_bit_for_bit(n, g):
    X = _pattern(n, g, seed=n + g)
    D = mo.jaccard_distance_matrix(X)
    D2 = mo.jaccard_distance_rows(X)
    assert D2.dtype == np.float64 and D2.tobytes() == D.tobytes()
    rows = np.random.RandomState(1).permutation(n)[: max(1, n // 3)]
    assert mo.jaccard_distance_rows(X, rows).tobytes() == np.ascontiguousarray(D[rows]).tobytes()
    inter, union = mo.jaccard_pair_counts(X, rows)
    B = X != 0
    Bi = B.astype(np.int64)
    assert np.array_equal(inter, Bi[rows] @ Bi.T)
    assert np.array_equal(union, (B[rows][:, None, :] | B[None, :, :]).sum(axis=2))


@pytest.mark.parametrize("n,g", [(5, 1), (9, 63), (20, 64), (20, 65), (50, 1000)])
def test_pair_counts_equal_popcounts_of_the_packed_words(n, g):
    from scrna_seq_qannealing_clustering_amd import metrics
    X = _pattern(n, g, seed=3 * n + g)
    bits = metrics.pack_expression(X)
    inter, union = mo.jaccard_pair_counts(X)
    assert np.array_equal(inter, np.bitwise_count(bits[:, None, :] & bits[None, :, :]).sum(axis=2, dtype=np.int64))
    assert np.array_equal(union, np.bitwise_count(bits[:, None, :] | bits[None, :, :]).sum(axis=2, dtype=np.int64))
