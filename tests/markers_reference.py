"""CPU reference of the rank-sum pass (``metrics.rank_sum_pass``): numpy and scipy only, one gene at a time.

Per gene ``scipy.stats.rankdata`` gives the midranks among all n cells (-0.0 and +0.0 compare equal, as floats do);
``np.rint(2 r)`` is summed per cluster with ``np.add.at``; the tie term is the sum of t^3 - t over the counts of
``np.unique``; the sums are one sequential fp64 ``np.add.at`` in cell order."""
import numpy as np
from scipy.stats import rankdata


def reference_stats(X, L, K, plain=False):
    """X: (n, g) float32; L: (B, n) labels in [0, K).  -> rank2 (B, g, K) int64, npos (B, g, K) int32, sums (B, g, K)
    float64, tie (g,) int64, sizes (B, K) int64"""
    X = np.asarray(X, dtype=np.float32)
    L = np.asarray(L).reshape(-1, X.shape[0]).astype(np.int64)
    (n, g), B = X.shape, L.shape[0]
    rank2 = np.zeros((B, g, K), dtype=np.int64)
    npos = np.zeros((B, g, K), dtype=np.int32)
    sums = np.zeros((B, g, K), dtype=np.float64)
    tie = np.zeros(g, dtype=np.int64)
    for j in range(g):
        x = X[:, j]
        r2 = np.rint(2.0 * rankdata(x)).astype(np.int64)
        t = np.unique(x, return_counts=True)[1].astype(np.int64)
        tie[j] = int((t ** 3 - t).sum())
        v = x.astype(np.float64) if plain else np.expm1(x.astype(np.float64))
        pos = (x > 0).astype(np.int32)
        for b in range(B):
            np.add.at(rank2[b, j], L[b], r2)
            np.add.at(npos[b, j], L[b], pos)
            np.add.at(sums[b, j], L[b], v)
    sizes = np.stack([np.bincount(L[b], minlength=K) for b in range(B)]).astype(np.int64)
    return rank2, npos, sums, tie, sizes


def sparse_matrix(rng, n, g, rate=0.3):
    """scRNA-like columns: a Poisson(rate) mask (about 26 % non-zero at 0.3) times uniform values"""
    return ((rng.poisson(rate, (n, g)) > 0) * rng.uniform(0.1, 4.0, (n, g))).astype(np.float32)
