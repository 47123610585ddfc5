"""Marker-gene detection on the GPU (mi_rank_sum_markers_f32, csrc/markers_kernels.hip) against the CPU reference of
tests/markers_reference.py (``scipy.stats.rankdata`` per gene).  Rank sums, counts and the tie term are exact integers and
are compared with ``np.array_equal``, in the LDS form of the ranking pass and in the forced HBM form, which must also
equal each other: the sizes where the wavefront, the workgroup and the transpose tile end, special columns (all zero, no
zero, one tie group, all distinct, heavy ties, negatives, both zeros, the ends of the sort's padding), labellings (K = 1,
K = 64 with unused labels, one labelling, one more than the kernel's chunk, identical rows, arbitrary cluster ids), the LDS
cap; the fp64 sums (bit for bit when plain, 1e-9 with expm1, identical between runs); and ``find_all_markers`` end to end
on a planted matrix, every p-value against ``scipy.stats.mannwhitneyu``, and on the labels of a resolution sweep."""
import numpy as np
import pytest
from scipy.stats import mannwhitneyu

from markers_reference import TIE_BLOCKS, reference_stats, sparse_matrix, tie_block_vectors
from test_gpu_modularity import graph
from scrna_seq_qannealing_clustering_amd import metrics
from scrna_seq_qannealing_clustering_amd.clustering import clustering_modularity_sweep

pytestmark = pytest.mark.gpu

RTOL = 1e-9                                   # the project's fp64 tolerance (tests/test_gpu_components.py)
P_RTOL = 1e-12
CAP = metrics.MARKERS_LDS_MAX_NONZEROS
CHUNK = metrics.MARKERS_LABELLING_CHUNK


def check_integers(X, L, K, forms=(False, True)):
    """both forms of the ranking pass against the reference, and against each other; -> the unforced result"""
    L = np.asarray(L).reshape(-1, X.shape[0])
    rank2, npos, _, tie, _ = reference_stats(X, L, K)
    out = []
    for force in forms:
        r = metrics.rank_sum_pass(X, L, K, force_global=force)
        assert r["rank2"].shape == (L.shape[0], X.shape[1], K)
        assert np.array_equal(r["rank2"], rank2), "rank2 (force_global=%s)" % force
        assert np.array_equal(r["npos"], npos), "npos (force_global=%s)" % force
        assert np.array_equal(r["tie"], tie), "tie (force_global=%s)" % force
        out.append(r)
    for r in out[1:]:
        for key in ("rank2", "npos", "tie", "sum"):
            assert np.array_equal(out[0][key], r[key]), key
    return out[0]


# ---- 1. wavefront, workgroup and tile edges -----------------------------------------------------------------------------

@pytest.mark.parametrize("g", [1, 63, 65])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_edges(n, g):
    rng = np.random.default_rng(1000 * n + g)
    X = sparse_matrix(rng, n, g)
    check_integers(X, rng.integers(0, 3, (2, n)), 3)


# ---- 2. special columns -------------------------------------------------------------------------------------------------

def special_columns(rng, n=300):
    cols = {
        "all_zero": np.zeros(n),
        "no_zeros": rng.uniform(0.5, 3.0, n),
        "one_tie_group": np.full(n, 1.25),
        "all_distinct": rng.permutation(n) + 1.0,
        "counts_0_3": rng.integers(0, 4, n).astype(float),
        "normal": rng.standard_normal(n),
        "both_zeros": np.where(rng.random(n) < 0.2, 1.5, np.where(rng.random(n) < 0.5, -0.0, 0.0)),
    }
    cols["both_zeros"][:4] = [-0.0, 0.0, -2.0, 2.0]
    for m in (255, 256, 257):
        c = np.zeros(n)
        c[rng.permutation(n)[:m]] = rng.uniform(0.1, 2.0, m)
        cols["nonzeros_%d" % m] = c
    return list(cols), np.stack(list(cols.values()), axis=1).astype(np.float32)


def test_special_columns():
    rng = np.random.default_rng(2)
    names, X = special_columns(rng)
    z = X[:, names.index("both_zeros")]
    assert np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()
    assert [int((X[:, names.index("nonzeros_%d" % m)] != 0).sum()) for m in (255, 256, 257)] == [255, 256, 257]
    r = check_integers(X, rng.integers(0, 5, (3, 300)), 5)
    n = 300
    assert r["tie"][names.index("all_zero")] == r["tie"][names.index("one_tie_group")] == n ** 3 - n
    assert r["tie"][names.index("all_distinct")] == 0
    # every gene's doubled ranks add up to n (n + 1), whatever the labelling
    assert (r["rank2"].sum(axis=2) == n * (n + 1)).all()


def test_tie_blocks_at_both_ends():
    """tie runs at sorted position 0 and at the last one, across position 256 and longer than a workgroup, in both forms"""
    rng = np.random.default_rng(11)
    V, runs = tie_block_vectors(rng)
    n = V.shape[1]
    for v, want in zip(V, runs):
        assert np.unique(v[v != 0], return_counts=True)[1].tolist() == want and sorted(want) == sorted(2 * TIE_BLOCKS)
        assert (v == 0).sum() == 16 and np.signbit(v[v == 0]).sum() == 8
    assert [(r[0], r[-1]) for r in runs] == [(1, 257), (257, 1), (2, 2)]
    r = check_integers(np.ascontiguousarray(V.T), rng.integers(0, 4, (2, n)), 4)
    assert r["tie"].tolist() == [2 * sum(t ** 3 - t for t in TIE_BLOCKS) + 16 ** 3 - 16] * 3


# ---- 3. labellings -------------------------------------------------------------------------------------------------------

def test_one_cluster_and_one_labelling():
    rng = np.random.default_rng(3)
    X = sparse_matrix(rng, 130, 9)
    r = check_integers(X, np.zeros(130, dtype=int), 1)
    assert (r["rank2"] == 130 * 131).all()


def test_64_clusters_with_unused_labels():
    rng = np.random.default_rng(4)
    X = sparse_matrix(rng, 200, 7)
    L = rng.choice([0, 5, 31, 62, 63], (2, 200))
    r = check_integers(X, L, 64)
    unused = np.setdiff1d(np.arange(64), [0, 5, 31, 62, 63])
    assert not r["rank2"][:, :, unused].any() and not r["npos"][:, :, unused].any() and not r["sum"][:, :, unused].any()


def test_one_more_labelling_than_the_chunk_and_identical_rows():
    rng = np.random.default_rng(5)
    n = 150
    X = sparse_matrix(rng, n, 11)
    X[:, 3] = rng.standard_normal(n)
    L = rng.integers(0, 6, (CHUNK + 1, n))
    L[CHUNK] = L[0]                                                  # the row past the chunk repeats the first
    L[7] = L[2]
    r = check_integers(X, L, 6)
    for key in ("rank2", "npos", "sum"):
        assert np.array_equal(r[key][CHUNK], r[key][0]) and np.array_equal(r[key][7], r[key][2]), key


def test_arbitrary_cluster_ids():
    rng = np.random.default_rng(6)
    n = 120
    X = sparse_matrix(rng, n, 8)
    lab = rng.integers(0, 3, n)
    a = metrics.find_all_markers(X, lab)
    b = metrics.find_all_markers(X, np.array([-7, 40, 1000])[lab])
    assert b["cluster_ids"].tolist() == [-7, 40, 1000] and a["cluster_ids"].tolist() == [0, 1, 2]
    for key in ("U", "p_val", "p_val_adj", "pct_1", "pct_2", "avg_log2FC", "auc", "passed", "cluster_size"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    assert a["U"].shape == (8, 3) and a["genes"].tolist() == list(range(8))


# ---- 4. the LDS cap ------------------------------------------------------------------------------------------------------

def test_lds_cap_in_one_call():
    rng = np.random.default_rng(7)
    n = CAP + 16
    X = np.zeros((n, 3), dtype=np.float32)
    for j, m in enumerate((CAP, CAP + 1, 10)):                      # the last LDS gene, the first HBM gene, a sparse one
        X[rng.permutation(n)[:m], j] = np.round(rng.uniform(0.1, 3.0, m), 2)      # (two decimals: ties among the non-zeros)
    assert (X != 0).sum(axis=0).tolist() == [CAP, CAP + 1, 10]
    check_integers(X, rng.integers(0, 4, (2, n)), 4)


# ---- 5. the sums ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [2, CHUNK + 1])                        # few labellings read X, many read its transpose
def test_sums(B):
    rng = np.random.default_rng(8 + B)
    n, g, K = 257, 65, 5
    X = sparse_matrix(rng, n, g)
    L = rng.integers(0, K, (B, n))
    want = reference_stats(X, L, K)[2]
    r = metrics.rank_sum_pass(X, L, K)
    assert np.allclose(r["sum"], want, rtol=RTOL, atol=0.0)
    assert np.array_equal(metrics.rank_sum_pass(X, L, K)["sum"], r["sum"])       # run to run
    Xs = X.copy()
    Xs[:, ::2] = rng.standard_normal((n, len(range(0, g, 2))))     # scaled data: negatives
    want = reference_stats(Xs, L, K, plain=True)[2]
    r = metrics.rank_sum_pass(Xs, L, K, plain=True)
    assert np.array_equal(r["sum"], want)                            # the same additions in the same order
    assert np.array_equal(metrics.rank_sum_pass(Xs, L, K, plain=True, force_global=True)["sum"], want)


# ---- 6. end to end -------------------------------------------------------------------------------------------------------

def planted(rng, n=512, g=200, K=4, per=10):
    lab = rng.permutation(np.arange(n) % K)
    X = sparse_matrix(rng, n, g)
    for c in range(K):
        cells = np.flatnonzero(lab == c)
        block = X[np.ix_(cells, np.arange(c * per, (c + 1) * per))]
        X[np.ix_(cells, np.arange(c * per, (c + 1) * per))] = np.where(rng.random(block.shape) < 0.9, block + 3.0, block)
    return X, lab


def test_find_all_markers_on_planted_clusters():
    rng = np.random.default_rng(9)
    X, lab = planted(rng)
    n, g = X.shape
    names = np.array(["g%03d" % j for j in range(g)])
    r = metrics.find_all_markers(X, lab + 10, only_pos=True, min_pct=0.25, logfc_threshold=0, genes=names)
    assert r["cluster_ids"].tolist() == [10, 11, 12, 13]
    top = metrics.top_markers(r, n=2)
    for c in range(4):
        assert len(top[10 + c]) == 2 and set(top[10 + c]) <= set(names[c * 10:(c + 1) * 10]), (c, top[10 + c])
    for j in range(g):
        for c in range(4):
            want = mannwhitneyu(X[lab == c, j], X[lab != c, j], use_continuity=True, method="asymptotic")
            assert r["U"][j, c] == want.statistic
            assert abs(r["p_val"][j, c] - want.pvalue) <= P_RTOL * want.pvalue, (j, c, r["p_val"][j, c], want.pvalue)
    assert np.array_equal(r["p_val_adj"], np.minimum(1.0, r["p_val"] * g))
    assert r["passed"][:10, 0].all() and not r["passed"][:10, 1:].any()      # only_pos: a planted gene marks its own cluster


def test_sweep_labels_in_one_call():
    G = graph("noisy_circles")
    sets = clustering_modularity_sweep(G, [0.5, 1, 2], 8, sampler_kwargs=dict(num_reads=16, num_sweeps=60, seed=3))
    L = np.stack([np.asarray(ss.record["sample"][0]) for ss in sets])
    n = L.shape[1]
    X = sparse_matrix(np.random.default_rng(10), n, 40)
    many = metrics.find_all_markers(X, L)
    assert many["U"].shape == (3, 40, len(many["cluster_ids"]))
    for b in range(3):
        one = metrics.find_all_markers(X, L[b])
        cols = np.searchsorted(many["cluster_ids"], one["cluster_ids"])
        assert np.array_equal(many["cluster_size"][b, cols], one["cluster_size"])
        assert many["cluster_size"][b].sum() == n
        for key in ("U", "pct_1", "passed"):
            assert np.array_equal(many[key][b][:, cols], one[key], equal_nan=True), key
        for key in ("p_val", "p_val_adj", "pct_2", "auc"):
            assert np.allclose(many[key][b][:, cols], one[key], rtol=1e-12, atol=0.0, equal_nan=True), key
        # (the other cells' sum is a total over K columns minus the cluster's: its last bit may depend on K)
        assert np.allclose(many["avg_log2FC"][b][:, cols], one["avg_log2FC"], rtol=1e-12, atol=1e-12, equal_nan=True)
