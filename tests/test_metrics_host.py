"""The host side of the cluster-quality metrics without a GPU: `metrics.pack_expression` (bit order, gene counts
that are not multiples of 64) and the closed forms of `metrics.cluster_stats`, fed the device pass's sufficient
statistics from a numpy stand-in built on the oracle's distance matrix.  CPU only."""
import numpy as np
import pytest

from oracle import metrics_oracle as mo
from scrna_seq_qannealing_clustering_amd import metrics
from test_gpu_metrics import SCALARS, VECTORS, expression


def unpack_bits(bits, g):
    """(n, W) uint64 -> (n, g) bool, one bit at a time: gene 64 w + b is bit b of word w."""
    n, W = bits.shape
    out = np.zeros((n, W * 64), dtype=bool)
    for w in range(W):
        for b in range(64):
            out[:, 64 * w + b] = (bits[:, w] >> np.uint64(b)) & np.uint64(1)
    assert not out[:, g:].any(), "padding bits must be zero"
    return out[:, :g]


@pytest.mark.parametrize("g", [1, 63, 64, 65, 128, 3001])
def test_pack_expression_bit_order_padding_and_dtypes(g):
    rng = np.random.RandomState(g)
    n = 37
    X = ((rng.rand(n, g) < 0.3) * (rng.rand(n, g) + 0.5)).astype(np.float32)
    X[:, g - 1] = 1.0                                           # the last gene: the highest used bit of the last word
    X[5] = 0
    bits = metrics.pack_expression(X)
    assert bits.dtype == np.uint64 and bits.shape == (n, (g + 63) // 64) and bits.flags["C_CONTIGUOUS"]
    assert np.array_equal(unpack_bits(bits, g), X != 0)
    assert (bits[:, -1] >> np.uint64((g - 1) % 64) == 1).sum() == n - 1      # nothing above gene g - 1 (row 5 is empty)
    for Y in (np.ceil(X).astype(np.int64), X != 0, X.astype(np.float64), -X):
        assert np.array_equal(metrics.pack_expression(Y), bits), Y.dtype


def numpy_pass(g):
    """A stand-in for metrics.jaccard_pass: the same outputs from the oracle's fp64 distance matrix in numpy."""
    def run(bits, labels, K, device=0, return_distances=False):
        lab = np.asarray(labels)
        n = len(lab)
        D = mo.jaccard_distance_matrix(unpack_bits(np.asarray(bits), g))
        member = lab[:, None] == np.arange(K)[None, :]                       # n x K
        same = lab[:, None] == lab[None, :]
        diam = np.zeros(K)
        sep = np.full((K, K), np.inf)
        for c in range(K):
            for c2 in range(K):
                blk = D[np.ix_(member[:, c], member[:, c2])]
                if blk.size and c == c2:
                    diam[c] = blk.max()
                elif blk.size:
                    sep[c, c2] = blk.min()
        np.fill_diagonal(sep, 0.0)
        return {"rowsum": D @ member.astype(np.float64), "sq_all": (D * D).sum(axis=1),
                "sq_within": (D * D * same).sum(axis=1), "diameter": diam, "separation.matrix": sep,
                "distances": D.astype(np.float32) if return_distances else None, "kernel_ms": 0.0}
    return run


def check_closed_forms(monkeypatch, X, labels):
    monkeypatch.setattr(metrics, "jaccard_pass", numpy_pass(X.shape[1]))
    st = metrics.cluster_stats(X, labels, return_distances=True)
    uniq, lab = np.unique(labels, return_inverse=True)
    D = mo.jaccard_distance_matrix(X)
    with np.errstate(all="ignore"):
        ref = mo.cluster_stats(D, lab)
    assert st["cluster.ids"].tolist() == uniq.tolist()
    assert np.array_equal(st["distances"], D.astype(np.float32))
    assert st["n"] == ref["n"] and st["cluster.number"] == ref["cluster.number"]
    assert st["n.within"] == ref["n.within"] and st["n.between"] == ref["n.between"]
    assert st["min.cluster.size"] == ref["min.cluster.size"]
    for k in VECTORS:
        assert np.shape(st[k]) == np.shape(ref[k]), k
        assert np.allclose(st[k], ref[k], rtol=1e-12, atol=1e-12, equal_nan=True), k
    assert np.array_equal(st["within.average.distance"], st["average.distance"], equal_nan=True)
    for k in SCALARS:
        assert np.isclose(st[k], ref[k], rtol=1e-10, atol=1e-12, equal_nan=True), (k, st[k], ref[k])
    return st, ref


# the shapes of test_gpu_metrics.test_cluster_stats_equal_oracle with fewer cells and genes
@pytest.mark.parametrize("n,g,K", [(90, 150, 4), (130, 64, 9), (65, 200, 2), (160, 301, 15), (40, 7, 1)])
def test_closed_forms_equal_oracle(monkeypatch, n, g, K):
    X, groups = expression(n, g, seed=n + g)
    labels = np.random.RandomState(K).randint(0, K, size=n) if K != 4 else groups
    labels[:K] = np.arange(K)
    check_closed_forms(monkeypatch, X, labels)


def test_closed_forms_arbitrary_ids_singleton_and_empty_rows(monkeypatch):
    X, _ = expression(120, 90, seed=5)
    X[3] = 0
    X[77] = 0
    labels = np.array([17, 203, 5, 88])[np.random.RandomState(2).randint(0, 4, size=120)]
    labels[10] = 999
    st, _ = check_closed_forms(monkeypatch, X, labels)
    assert st["sil.widths"][10] == 0.0 and np.isnan(st["average.distance"][-1]) and st["diameter"][-1] == 0.0


def test_closed_forms_one_cluster(monkeypatch):
    X, _ = expression(30, 40, seed=8)
    st, _ = check_closed_forms(monkeypatch, X, np.full(30, 7))
    assert st["n.between"] == 0 and np.isnan(st["average.between"]) and np.isnan(st["wb.ratio"])
    assert np.isnan(st["pearsongamma"]) and np.isnan(st["ch"]) and np.isnan(st["dunn2"])
    assert st["min.separation"] == np.inf and np.all(st["sil.widths"] == 0.0) and st["entropy"] == 0.0


def test_closed_forms_all_singletons(monkeypatch):
    """K = n: no within-cluster pair exists.  Every diameter and within-cluster sum is 0, every average within-cluster
    distance is undefined (NaN), and so are dunn (max diameter 0), dunn2 (fpc: smallest average between-cluster
    dissimilarity over the largest average within-cluster dissimilarity, of which there is none), ch (wss = 0) and
    pearsongamma (the indicator is constant); product and oracle agree on all of them."""
    X, _ = expression(25, 60, seed=11)
    st, _ = check_closed_forms(monkeypatch, X, np.arange(25)[::-1].copy())
    assert st["n.within"] == 0 and st["within.cluster.ss"] == 0.0 and st["average.within"] == 0.0
    assert np.all(st["diameter"] == 0.0) and np.all(np.isnan(st["average.distance"]))
    assert np.all(st["sil.widths"] == 0.0) and st["wb.ratio"] == 0.0
    for k in ("dunn", "dunn2", "ch", "pearsongamma"):
        assert np.isnan(st[k]), k


def test_closed_forms_two_clusters_one_singleton(monkeypatch):
    X, _ = expression(21, 50, seed=13)
    labels = np.zeros(21, dtype=np.int64)
    labels[9] = 1
    st, _ = check_closed_forms(monkeypatch, X, labels)
    assert st["cluster.size"].tolist() == [20, 1] and st["sil.widths"][9] == 0.0
    assert np.isfinite(st["dunn2"]) and np.isfinite(st["ch"]) and np.isfinite(st["pearsongamma"])


def test_labels_must_match_cells():
    with pytest.raises(ValueError):
        metrics.cluster_stats(np.ones((4, 3)), np.zeros(5, dtype=int))
    with pytest.raises(ValueError):
        metrics.cluster_stats(np.ones((4, 3)), np.zeros((4, 1), dtype=int))
