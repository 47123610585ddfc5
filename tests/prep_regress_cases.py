"""What the regression and QC tests share (tests/test_prep_regress_model.py, tests/test_gpu_prep_regress.py): a numpy fp64
restatement of ``mi_prep_select_regressed`` stage by stage -- the residual with its multiply-adds unfused and k ascending, the
flat rule, the scaled matrix with one rounding to float32, so that ``Z`` can be compared with ``np.array_equal`` -- and the
generators: covariates, a matrix with flat columns, a CSR with stored zeros and an empty row, and the planted matrix with a
per-cell nuisance factor of the end-to-end checks."""
import numpy as np
import scipy.sparse as sp

import prep_reference as ref

FLAT_RTOL = 1e-16                             # flat_j = sum (r - mean)^2 <= FLAT_RTOL * sum y^2 (include/mi_prep.h)


def intercept_basis(n):
    """Q of the design [1]: one column 1 / sqrt(n)"""
    return np.full((n, 1), 1.0 / np.sqrt(n))


def coefficients(Y, Q):
    """-> c = Q^T Y (q x h), S = sum_i y^2 (h), in fp64 (numpy's order of addition)"""
    Y64 = np.asarray(Y, dtype=np.float32).astype(np.float64)
    return Q.T @ Y64, (Y64 * Y64).sum(axis=0)


def residuals(Y, Q, c):
    """r = y - acc, acc = Q_i0 c_0, then acc = acc + Q_ik c_k for k ascending: the device's expression, element by element"""
    Y64 = np.asarray(Y, dtype=np.float32).astype(np.float64)
    acc = Q[:, 0:1] * c[0][None, :]
    for k in range(1, Q.shape[1]):
        acc = acc + Q[:, k:k + 1] * c[k][None, :]
    return Y64 - acc


def moments(r, mean=None):
    """-> mean (sum / n) unless given, ss = sum (r - mean)^2, var = ss / (n - 1)"""
    n = r.shape[0]
    mean = r.sum(axis=0) / n if mean is None else mean
    ss = ((r - mean) ** 2).sum(axis=0)
    return mean, ss, ss / (n - 1)


def scaled(Y, Q, c, mean, var, flat, clip):
    """stage 5: z = flat ? 0 : f32(min((r - mean) * (1 / sqrt(var)), clip))"""
    flat = np.asarray(flat, dtype=bool)
    inv = np.where(flat, 0.0, 1.0 / np.sqrt(np.where(flat, 1.0, var)))
    z = np.minimum((residuals(Y, Q, c) - mean) * inv, clip).astype(np.float32)
    z[:, flat] = 0.0
    return z


def regress_scale(Y, Q, clip):
    """the whole entry in numpy -> Z (float32), c, mean, var, flat"""
    c, S = coefficients(Y, Q)
    mean, ss, var = moments(residuals(Y, Q, c))
    flat = ss <= FLAT_RTOL * S
    return scaled(Y, Q, c, mean, var, flat, clip), c, mean, var, flat


def percent_of_first_genes(X):
    """the covariate derived from the data: the cell's percent of counts in genes 0 .. g / 10 (at least one gene)"""
    X64 = np.asarray(X, dtype=np.float64)
    tot = X64.sum(axis=1)
    return 100.0 * X64[:, :max(X.shape[1] // 10, 1)].sum(axis=1) / np.where(tot > 0, tot, 1.0)


def covariates(rng, X, p):
    """(n, p): p - 1 standard normal columns and the percent column last"""
    return np.column_stack([rng.normal(size=(X.shape[0], p - 1)), percent_of_first_genes(X)])


FLAT_GENES = {"zero": 0, "constant": 1, "one_cell": 2, "in_span": 3, "filler": 19}


def flat_columns_counts(rng, n=257, g=20):
    """integer counts whose cells all have one total (gene `filler` makes it up), so that a constant count stays constant
    after normalisation: gene `zero` is all zero, `constant` is 3 everywhere, `one_cell` has a single non-zero cell; the
    covariate of the test is built from the normalised column of `in_span`"""
    X = ref.sparse_counts(rng, n, g)
    X[:, FLAT_GENES["zero"]] = 0.0
    X[:, FLAT_GENES["constant"]] = 3.0
    X[:, FLAT_GENES["one_cell"]] = 0.0
    X[5, FLAT_GENES["one_cell"]] = 7.0
    X[:, FLAT_GENES["filler"]] = 0.0
    tot = X.sum(axis=1)
    X[:, FLAT_GENES["filler"]] = tot.max() + 1.0 - tot
    assert len(set(X.sum(axis=1).tolist())) == 1
    return X


def csr_with_stored_zeros_and_empty_row(X, rng, share=0.1):
    """-> (the dense matrix with row 3 emptied, a csr of it that stores some of its zeros, none of them in row 3)"""
    X = X.copy()
    X[3] = 0.0
    pattern = (X != 0) | (rng.random(X.shape) < share)
    zeros = np.argwhere((X == 0) & (np.arange(X.shape[0]) != 3)[:, None])
    assert len(zeros) > 0
    pattern[tuple(zeros[0])] = True                              # (at least one, whatever the draw)
    pattern[3] = False
    rows, cols = np.nonzero(pattern)
    A = sp.csr_matrix((X[rows, cols], (rows, cols)), shape=X.shape)
    assert A.nnz == pattern.sum() > (X != 0).sum() and A.indptr[3] == A.indptr[4]
    return X, A


def planted_counts_with_nuisance(seed, n=ref.PLANTED_N, g=ref.PLANTED_G, fold=6.0, strength=1.5):
    """``prep_reference.planted_counts`` (the same draws in the same order), with the rates of genes 160 .. g - 1 multiplied,
    before the Poisson draw, by exp(strength (u_i - 0.5)), u ~ U(0, 1) per cell from default_rng(1000 + seed)
    -> (counts f32, groups, u)"""
    rng = np.random.default_rng(seed)
    sizes = [int(round(f * n)) for f in (0.4, 0.3, 0.2)]
    sizes.append(n - sum(sizes))
    groups = rng.permutation(np.repeat(np.arange(4), sizes))
    base = np.exp(rng.normal(-1.0, 1.0, g))
    rate = np.tile(base, (n, 1))
    for c in range(4):
        rate[np.ix_(groups == c, np.arange(40 * c, 40 * c + 40))] *= fold
    depth = rng.uniform(0.5, 2.0, n)
    u = np.random.default_rng(1000 + seed).uniform(0.0, 1.0, n)
    rate[:, 160:] *= np.exp(strength * (u - 0.5))[:, None]
    return rng.poisson(rate * depth[:, None]).astype(np.float32), groups, u


def pca_coords_all_genes(X, npcs, Q=None, clip=10.0):
    """the chain in numpy with every gene a feature: normalise, (regress,) scale, PCA -> coords (n x npcs, fp64), eigenvalues"""
    Y = ref.normalize(X)
    if Q is None:
        Z = ref.scaled_from_normalized(Y, np.arange(X.shape[1]), clip)
    else:
        Z = regress_scale(Y, Q, clip)[0]
    Z = Z.astype(np.float64)
    w, V = np.linalg.eigh(Z.T @ Z / (X.shape[0] - 1))
    w, V = w[::-1], V[:, ::-1]
    return Z @ V[:, :npcs], w


def knn_lists(P, k):
    """indices of the k nearest other points of every row of P (fp64, brute force)"""
    d = ((P[:, None, :] - P[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    return np.argsort(d, axis=1, kind="stable")[:, :k]


def max_abs_corr(coords, u):
    """-> |corr(coords[:, k], u)| per column"""
    a = coords - coords.mean(axis=0)
    b = u - u.mean()
    return np.abs(a.T @ b) / (np.linalg.norm(a, axis=0) * np.linalg.norm(b))
