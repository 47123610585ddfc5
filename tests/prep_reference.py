"""CPU reference of the preprocessing passes (``preprocess.ExpressionMatrix``): numpy only, fp64 throughout, except the
scaled matrix ``Z``, which is reproduced in numpy float32 with the kernel's exact expression (separate subtract and
multiply, then the minimum with the clip), so that it can be compared with ``np.array_equal``.  Also the generators the
tests share: scRNA-like counts and the planted four-group matrix of the end-to-end checks."""
import numpy as np


def normalize(X, scale_factor=1e4):
    """fp64 ``log1p(x * scale_factor / total)``, rounded once to float32; a cell whose total is 0 keeps zeros"""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    tot = X64.sum(axis=1, keepdims=True)
    safe = np.where(tot > 0, tot, 1.0)
    return np.where(tot > 0, np.log1p(X64 * scale_factor / safe), 0.0).astype(np.float32)


def gene_stats(M):
    """-> mean, variance (ddof 1, two passes), nnz per column of the float32 matrix M"""
    M64 = np.asarray(M, dtype=np.float32).astype(np.float64)
    n = M64.shape[0]
    mean = M64.sum(axis=0) / n
    var = ((M64 - mean) ** 2).sum(axis=0) / (n - 1)
    return mean, var, (M64 != 0).sum(axis=0).astype(np.int32)


def clipped_variance(X, mean, sd, clip):
    """sum_i min((x - mean) / sd, clip)^2 / (n - 1), 0 where sd == 0"""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    sd = np.asarray(sd, dtype=np.float64)
    ok = sd != 0
    out = np.zeros(X64.shape[1])
    s = np.minimum((X64[:, ok] - np.asarray(mean)[ok]) / sd[ok], clip)
    out[ok] = (s * s).sum(axis=0) / (X64.shape[0] - 1)
    return out


# ---- the column reductions restated in their own order: equal bit for bit, not within a tolerance ---------------------------
# include/mi_prep.h: inside a slice of ROW_SLICE rows, row lane ty adds the rows r0 + ty, r0 + ty + ROW_LANES, ... ascending;
# the lanes join as ((s0 + s1) + s2) + s3; the slices add in ascending order; one division.  All IEEE fp64, no contraction,
# so numpy's elementwise fp64 gives the same bits.
ROW_SLICE, ROW_LANES = 256, 4


def ordered_column_sum(T, denom=1.0):
    """the device's sum over the rows of the fp64 terms T (n x columns), divided once"""
    T = np.asarray(T, dtype=np.float64)
    total = np.zeros(T.shape[1])
    for r0 in range(0, T.shape[0], ROW_SLICE):
        r1 = min(r0 + ROW_SLICE, T.shape[0])
        lanes = []
        for ty in range(ROW_LANES):
            acc = np.zeros(T.shape[1])
            for r in range(r0 + ty, r1, ROW_LANES):
                acc = acc + T[r]
            lanes.append(acc)
        total = total + (((lanes[0] + lanes[1]) + lanes[2]) + lanes[3])
    return total / denom


def plain_column_sum(T, denom=1.0):
    """the rows added in ascending order into one accumulator: what the device does not do (the tests' control)"""
    T = np.asarray(T, dtype=np.float64)
    total = np.zeros(T.shape[1])
    for row in T:
        total = total + row
    return total / denom


def ordered_gene_stats(M, column_sum=ordered_column_sum):
    """gene_stats in the device's order -> mean, variance, nnz"""
    M64 = np.asarray(M, dtype=np.float32).astype(np.float64)
    n = M64.shape[0]
    mean = column_sum(M64, n)
    d = M64 - mean
    return mean, column_sum(d * d, n - 1), (M64 != 0).sum(axis=0).astype(np.int32)


def ordered_clipped_variance(X, mean, sd, clip):
    """clipped_variance in the device's order and operations: d = (x - mean) / sd, d < clip ? d : clip, d * d"""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    mean, sd = np.asarray(mean, dtype=np.float64), np.asarray(sd, dtype=np.float64)
    ok = sd != 0
    d = (X64 - mean) / np.where(ok, sd, 1.0)
    d = np.where(d < clip, d, clip)
    return ordered_column_sum(np.where(ok, d * d, 0.0), X64.shape[0] - 1)


def ordered_regression(Yg, Q, column_sum=ordered_column_sum):
    """select_regressed's fp64 outputs from the gathered float32 columns Yg (n x h) and the basis Q (n x q), in the device's
    order: c_k = sum_i Q_ik y_i; r = y - acc with acc = Q_i0 c_0, then acc = acc + Q_ik c_k; the mean of r; the squares about
    it over n - 1  ->  coef_q (q x h), resid_mean, resid_var"""
    Y64 = np.asarray(Yg, dtype=np.float32).astype(np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    n, q = Q.shape
    coef = np.stack([column_sum(Q[:, k:k + 1] * Y64) for k in range(q)])
    acc = Q[:, 0:1] * coef[0]
    for k in range(1, q):
        acc = acc + Q[:, k:k + 1] * coef[k]
    r = Y64 - acc
    mean = column_sum(r, n)
    d = r - mean
    return coef, mean, column_sum(d * d) / (n - 1)


def fractional_counts(rng, n, g):
    """non-negative float32 "counts" that are no integers, about 70 % zeros: a gamma draw times a power of two between
    2^-24 and 2^24 (integer counts, and float32 values of one magnitude, add exactly in fp64 and would pin no order); from
    three columns on, the last is all zero and the one before it constant"""
    X = (rng.gamma(2.0, 1.5, (n, g)) * 2.0 ** rng.integers(-24, 25, (n, g)) * (rng.random((n, g)) < 0.3)).astype(np.float32)
    if g >= 3:
        X[:, -1] = 0.0
        X[:, -2] = 0.3
    return X


def scaled(Y, genes, mu, sigma, clip):
    """the kernel's float32 expression: z = min((y - f32(mu)) * f32(1 / sigma), f32(clip)), 0 where sigma == 0"""
    Y = np.asarray(Y, dtype=np.float32)
    sigma = np.asarray(sigma, dtype=np.float64)
    flat = sigma == 0
    inv = (1.0 / np.where(flat, 1.0, sigma)).astype(np.float32)
    d = Y[:, np.asarray(genes)] - np.asarray(mu, dtype=np.float64).astype(np.float32)
    assert d.dtype == np.float32
    z = np.minimum(d * inv, np.float32(clip))
    z[:, flat] = 0.0
    return z.astype(np.float32)


def scaled_from_normalized(Y, genes, max_value=10.0):
    """ScaleData of the chosen columns: mu, sigma = mean and sd (ddof 1) of the normalised matrix"""
    mean, var, _ = gene_stats(Y)
    genes = np.asarray(genes)
    return scaled(Y, genes, mean[genes], np.sqrt(var[genes]), max_value)


def gram_bound(G64, terms):
    """|G - G64|_ab <= (terms + 2) 2^-24 sqrt(G64_aa G64_bb): an fmaf chain of `terms` products per chunk (standard
    summation bound), Cauchy-Schwarz over the chunk, again over the chunks; the fp64 adds are far below"""
    d = np.sqrt(np.maximum(np.diag(G64), 0.0))
    return (terms + 2) * 2.0 ** -24 * np.outer(d, d)


def project_bound(Z, V):
    """|out - Z64 V64|_ic <= (h + 2) 2^-24 |z_i| |v_c|"""
    Z64, V64 = np.asarray(Z, dtype=np.float64), np.asarray(V, dtype=np.float64)
    return (Z64.shape[1] + 2) * 2.0 ** -24 * np.outer(np.linalg.norm(Z64, axis=1), np.linalg.norm(V64, axis=0))


def variable_features(X, nfeatures, loess_fit, span=0.3):
    """vst on the counts with the given loess -> (genes in rank order, standardised variance)"""
    n = X.shape[0]
    mean, var, _ = gene_stats(X)
    ok = var > 0
    sd = np.zeros(len(mean))
    sd[ok] = np.sqrt(10.0 ** loess_fit(np.log10(mean[ok]), np.log10(var[ok]), span=span, degree=2))
    vs = clipped_variance(X, mean, sd, np.sqrt(n))
    return np.argsort(-vs, kind="stable")[:nfeatures], vs


def pca_coords(X, nfeatures, npcs, loess_fit, scale_factor=1e4, max_value=10.0):
    """the whole chain in numpy: -> coords (n x npcs, fp64), eigenvalues (all h, descending), genes"""
    Y = normalize(X, scale_factor)
    genes, _ = variable_features(X, nfeatures, loess_fit)
    Z = scaled_from_normalized(Y, genes, max_value).astype(np.float64)
    w, V = np.linalg.eigh(Z.T @ Z / (X.shape[0] - 1))
    w, V = w[::-1], V[:, ::-1]
    return Z @ V[:, :npcs], w, genes


def sparse_counts(rng, n, g, rate=0.3):
    """scRNA-like counts: a Poisson(rate) mask (about 26 % non-zero at 0.3) times counts of 1 .. 20"""
    return ((rng.poisson(rate, (n, g)) > 0) * rng.integers(1, 21, (n, g))).astype(np.float32)


PLANTED_N, PLANTED_G, PLANTED_FEATURES, PLANTED_PCS = 600, 400, 200, 10


def planted_counts(seed, n=PLANTED_N, g=PLANTED_G, fold=6.0):
    """4 groups of 40 / 30 / 20 / 10 % of the cells, shuffled; base rates exp(N(-1, 1)) per gene; genes 40 c .. 40 c + 39
    at `fold` times the base rate in group c; depth U(0.5, 2) per cell; Poisson(rate * depth).  -> (counts f32, groups)"""
    rng = np.random.default_rng(seed)
    sizes = [int(round(f * n)) for f in (0.4, 0.3, 0.2)]
    sizes.append(n - sum(sizes))
    groups = rng.permutation(np.repeat(np.arange(4), sizes))
    base = np.exp(rng.normal(-1.0, 1.0, g))
    rate = np.tile(base, (n, 1))
    for c in range(4):
        rate[np.ix_(groups == c, np.arange(40 * c, 40 * c + 40))] *= fold
    depth = rng.uniform(0.5, 2.0, n)
    return rng.poisson(rate * depth[:, None]).astype(np.float32), groups
