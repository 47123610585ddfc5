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


TIE_BLOCKS = (1, 2, 3, 64, 65, 257)


def tie_block_vectors(rng):
    """(3, 800) float32 vectors made of tie blocks only: every length of TIE_BLOCKS once among the negatives and once
    among the positives, one block of 16 zeros of both signs, the entries shuffled by position.  In ascending order of
    value vector 0 begins with the block of 1 and ends with the block of 257, vector 1 the other way round, vector 2
    begins and ends with a block of 2: tie runs that touch sorted position 0 and the last one, one longer than a workgroup
    of 256 that straddles position 256.  -> the vectors and, per vector, the run lengths of its non-zeros in sorted order"""
    out, runs = [], []
    for first, last in ((1, 257), (257, 1), (2, 2)):
        neg = [first] + [int(t) for t in rng.permutation([t for t in TIE_BLOCKS if t != first])]
        pos = [int(t) for t in rng.permutation([t for t in TIE_BLOCKS if t != last])] + [last]
        v = [np.full(t, -0.5 * (len(neg) - b)) for b, t in enumerate(neg)]
        v += [np.zeros(8), -np.zeros(8)]
        v += [np.full(t, 0.5 * (b + 1)) for b, t in enumerate(pos)]
        out.append(rng.permutation(np.concatenate(v)))
        runs.append(neg + pos)
    return np.stack(out).astype(np.float32), runs


def sparse_matrix(rng, n, g, rate=0.3):
    """scRNA-like columns: a Poisson(rate) mask (about 26 % non-zero at 0.3) times uniform values"""
    return ((rng.poisson(rate, (n, g)) > 0) * rng.uniform(0.1, 4.0, (n, g))).astype(np.float32)
