"""Inputs the sparse-preprocessing tests share (tests/test_prep_sparse_host.py, tests/test_gpu_prep_sparse.py): the three
generators of count matrices, the lane-ordered cell total the device computes, and the fp64 closed forms a matrix too
large to densify is checked against."""
import numpy as np
import scipy.sparse as sp

import prep_reference as ref


def counts_dense_rate(rng, n, g):
    return ref.sparse_counts(rng, n, g, rate=0.3)


def counts_thin(rng, n, g):
    """about 2 % non-zero: whole row slices and columns are empty"""
    return ref.sparse_counts(rng, n, g, rate=0.02)


def counts_wide_range(rng, n, g):
    """about 26 % non-zero, each uniform(1, 2) * 2^e with e uniform in -20 .. 20: fp64 sums of such float32 values round,
    so the order of the additions shows in the last bits (sums of small integer counts are exact in any order)"""
    mask = rng.poisson(0.3, (n, g)) > 0
    vals = rng.uniform(1.0, 2.0, (n, g)) * 2.0 ** rng.integers(-20, 21, (n, g))
    return (mask * vals).astype(np.float32)


GENERATORS = {"rate0.3": counts_dense_rate, "rate0.02": counts_thin, "wide": counts_wide_range}


def left_to_right_total(row):
    """fp64 sum of a cell's non-zeros in column order"""
    t = 0.0
    for v in row[row != 0]:
        t += float(v)
    return t


def lane_ordered_total(row):
    """the device's order: lane l adds columns l, l + 64, ... ascending, then the butterfly of wave_sum_f64 (offsets 32, 16,
    ... 1; lane l takes v[l] + v[l ^ off])"""
    lanes = np.zeros(64)
    for j, v in enumerate(row):
        lanes[j & 63] += float(v)
    off = 32
    while off:
        lanes = lanes + lanes[np.arange(64) ^ off]
        off >>= 1
    return float(lanes[0])


def with_stored_zeros(X, rng, share=0.1):
    """csr of the dense X with some of its zeros stored explicitly"""
    pattern = (X != 0) | (rng.random(X.shape) < share)
    rows, cols = np.nonzero(pattern)
    A = sp.csr_matrix((X[rows, cols], (rows, cols)), shape=X.shape)
    assert A.nnz == pattern.sum() and A.has_canonical_format
    return A


def closed_form_stats(A):
    """per gene of a csr/csc matrix in fp64, touching the stored entries only: mean = sum / n, var = (sum_nz (v - m)^2 +
    (n - nnz) m^2) / (n - 1), nnz = values != 0"""
    C = sp.csc_matrix(A).astype(np.float64)
    n = C.shape[0]
    mean = np.asarray(C.sum(axis=0)).ravel() / n
    col = np.repeat(np.arange(C.shape[1]), np.diff(C.indptr))
    nz = np.bincount(col, weights=(C.data != 0), minlength=C.shape[1])
    dev = np.bincount(col, weights=np.where(C.data != 0, (C.data - mean[col]) ** 2, 0.0), minlength=C.shape[1])
    return mean, (dev + (n - nz) * mean ** 2) / (n - 1), nz.astype(np.int32)


def closed_form_clipped(A, mean, sd, clip):
    """sum_i min((x - mean) / sd, clip)^2 / (n - 1), 0 where sd == 0, from the stored entries and the count of zeros"""
    C = sp.csc_matrix(A).astype(np.float64)
    n = C.shape[0]
    col = np.repeat(np.arange(C.shape[1]), np.diff(C.indptr))
    ok = sd != 0
    safe = np.where(ok, sd, 1.0)
    nzmask = C.data != 0
    nz = np.bincount(col, weights=nzmask, minlength=C.shape[1])
    s = np.minimum((C.data - mean[col]) / safe[col], clip) ** 2
    tot = np.bincount(col, weights=np.where(nzmask, s, 0.0), minlength=C.shape[1])
    zero = np.minimum((0.0 - mean) / safe, clip) ** 2
    return np.where(ok, (tot + (n - nz) * zero) / (n - 1), 0.0)
