"""Annotation on the resident expression handle: the numpy restatement of the per-cluster means (DESIGN.md section 5c,
"Annotation on the resident handle") and the small matrices the host and GPU tests share.  Host only."""
import functools

import numpy as np
import scipy.sparse as sp

import annot_cases
from scrna_seq_qannealing_clustering_amd import annotate

N = 70                                                           # cells of every matrix here
M_LIST = (1, 63, 64, 65, 130)
K_LIST = (1, 2, 65, N)
ZERO_CELL, EMPTY_GENE, LONG_ROW = 5, 7, 3
# Four values whose fp64 sum depends on the order at a place the fp32 mean shows, when the cluster's size is a power of two:
# one after another, 1 + 2^-24 absorbs each 2^-53 (a tie, to even), and the mean is a tie between two fp32 values that goes
# down; any order that adds the two small values to each other first (a pairwise or tree sum) ends one fp64 ulp higher, and
# the mean goes up.  interleaved_labels(2) puts the cells 0 .. 3 into a cluster of 64.
ORDER_SENSITIVE = np.array([1.0, 2.0 ** -24, 2.0 ** -53, 2.0 ** -53], dtype=np.float32)


def cluster_means_reference(X, cols, cluster_of):
    """-> (means (K, m) float32, sizes (K,) int32), K = max(cluster_of) + 1.  ``means[c, s]`` is the fp64 sum of
    ``float64(X[i, cols[s]])`` over the cells of cluster c in ascending cell index, one addition after another
    (``np.cumsum`` along the cells: ``np.sum`` adds pairwise), divided by the cluster's size, rounded to fp32."""
    X = np.asarray(X)
    cols = np.asarray(cols, dtype=np.int64)
    of = np.asarray(cluster_of, dtype=np.int64)
    K = int(of.max()) + 1
    means, sizes = np.empty((K, len(cols)), dtype=np.float32), np.empty(K, dtype=np.int32)
    for c in range(K):
        rows = X[of == c][:, cols].astype(np.float64)
        sizes[c] = rows.shape[0]
        means[c] = (np.cumsum(rows, axis=0)[-1] / np.float64(rows.shape[0])).astype(np.float32)
    return means, sizes


def pairwise_means(X, cols, cluster_of):
    """the same means with ``np.sum`` over each gene's contiguous values (pairwise): what an order-blind reduction gives"""
    X = np.asarray(X)
    of = np.asarray(cluster_of, dtype=np.int64)
    K = int(of.max()) + 1
    out = np.empty((K, len(cols)), dtype=np.float32)
    for c in range(K):
        genes = np.ascontiguousarray(X[of == c][:, np.asarray(cols, dtype=np.int64)].astype(np.float64).T)
        out[c] = (np.sum(genes, axis=1) / np.float64(genes.shape[1])).astype(np.float32)
    return out


@functools.lru_cache(maxsize=None)
def matrix(name):
    """float32 counts, about 10 % non-zeros.  "base": 70 x 300, cell ZERO_CELL all zero, gene EMPTY_GENE without entries,
    the last gene ORDER_SENSITIVE in the cells 0 .. 3 and zero elsewhere.
    "wide": 70 x 1200, row LONG_ROW with 700 non-zeros (past one pass of a 256-thread workgroup)."""
    g = {"base": 300, "wide": 1200}[name]
    rng = np.random.default_rng(g)
    X = (rng.integers(1, 40, (N, g)) * (rng.random((N, g)) < 0.10)).astype(np.float32)
    X[ZERO_CELL] = 0.0
    X[:, EMPTY_GENE] = 0.0
    if name == "base":                                           # (see ORDER_SENSITIVE)
        X[:, g - 1] = 0.0
        X[:4, g - 1] = ORDER_SENSITIVE
    if name == "wide":
        X[LONG_ROW] = 0.0
        X[LONG_ROW, np.sort(rng.choice(np.delete(np.arange(g), EMPTY_GENE), 700, replace=False))] = rng.integers(1, 40, 700)
    X.setflags(write=False)
    return X


def marker_cols(g, m, seed=0):
    """m distinct genes of g, shuffled (not ascending); genes 0 and g - 1 are among them from m = 2, EMPTY_GENE from m = 3"""
    rng = np.random.default_rng(1000 * m + g + seed)
    fixed = [0, g - 1, EMPTY_GENE][:m]
    rest = np.setdiff1d(np.arange(g), fixed)
    cols = np.concatenate([fixed, rng.choice(rest, m - len(fixed), replace=False)]).astype(np.int32)
    cols = rng.permutation(cols)
    if m > 2:
        assert (np.diff(cols) < 0).any()
    return cols


def csr_with_stored_zeros(X, cols):
    """X as CSR with a few explicitly stored zeros on the genes ``cols`` (never on EMPTY_GENE, which keeps no entry)"""
    rng = np.random.default_rng(X.shape[1])
    rows, genes = (list(v) for v in np.nonzero(X))
    stored = len(rows)
    for j in [int(c) for c in cols if c != EMPTY_GENE][:6]:
        for i in rng.choice(np.flatnonzero(X[:, j] == 0), 3, replace=False):
            rows.append(int(i))
            genes.append(j)
    data = np.concatenate([X[rows[:stored], genes[:stored]], np.zeros(len(rows) - stored)]).astype(np.float32)
    out = sp.csr_matrix((data, (rows, genes)), shape=X.shape)
    assert out.nnz == len(rows) > stored and np.array_equal(out.toarray(), X)
    return out


def interleaved_labels(K):
    """cluster ids of the N cells for K in K_LIST, interleaved (not sorted), every id used.  K = 2: every twelfth cell from
    ZERO_CELL on is cluster 1, the other 64 cells cluster 0; K = 65: cluster 64 is the single cell N - 1 (the ids go past one
    wavefront of cluster lanes); K = N: every cell its own cluster, in a shuffled order."""
    if K == 2:
        lab = np.zeros(N, dtype=np.int32)
        lab[ZERO_CELL::12] = 1
        return lab
    if K == N:
        return np.random.default_rng(K).permutation(N).astype(np.int32)
    if K == 65:
        lab = (np.arange(N) % 64).astype(np.int32)
        lab[N - 1] = 64
        return lab
    return (np.arange(N) % K).astype(np.int32)


@functools.lru_cache(maxsize=None)
def planted():
    """annot_cases.planted at L = 3 on g = 300 genes named as the "base" matrix's (label 2 the near-twin of label 0, so
    fine-tuning iterates), with its Reference (de_n = 25: about a hundred markers)"""
    c = annot_cases.planted(L=3, per_label=4, g=300, n=N, seed=31, twins=1, up=25, extra_ref_genes=20, drop=15)
    c.ref = annotate.Reference(c.R, c.ref_gene_names, c.ref_labels, de_n=25)
    return c
