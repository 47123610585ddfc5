"""numpy fp64 restatement of SCTransform's corrected counts (include/mi_prep.h, ``mi_prep_sct_correct``) and the inputs the
tests of it share (tests/test_sct_correct_host.py, tests/test_gpu_sct_correct.py).

Corrected counts are integers, so device and restatement are compared for EQUALITY.  An ``exp`` that differs from numpy's by
an ulp can flip an entry only where ``mu_r + r s_r`` lies next to a half-integer: :func:`near_half` marks the entries within
``HALF_TOL`` of one, and every test asserts that its inputs have none."""
import functools

import numpy as np

import prep_reference as ref

HALF_TOL = 1e-9


def value(x, mu, alpha, mu_r):
    """``mu_r + r s_r`` before rounding: the unclipped Pearson residual of x carried to the reference mean (separate multiply
    and add, as the device's)"""
    x, mu, alpha, mu_r = (np.asarray(a, dtype=np.float64) for a in (x, mu, alpha, mu_r))
    s = np.sqrt(mu + alpha * (mu * mu))
    s_r = np.sqrt(mu_r + alpha * (mu_r * mu_r))
    r = (x - mu) / s
    return mu_r + r * s_r


def count_of(v):
    """``fmax(rint(v), 0)``, half to even"""
    return np.maximum(np.rint(v), 0.0)


def near_half(v, tol=HALF_TOL):
    """is v within tol of some k + 0.5"""
    return np.abs(np.abs(v - np.floor(v)) - 0.5) <= tol


def values(X, b0, b1, alpha, log_umi, log_umi_ref):
    """(n x len(b0)) ``mu_r + r s_r`` of the columns of X, in order, under their parameters"""
    b0, b1, alpha, lu = (np.asarray(a, dtype=np.float64) for a in (b0, b1, alpha, log_umi))
    mu = np.exp(b0[None, :] + b1[None, :] * lu[:, None])
    mu_r = np.exp(b0 + b1 * float(log_umi_ref))
    return value(np.asarray(X, dtype=np.float32).astype(np.float64), mu, alpha[None, :], mu_r[None, :])


def corrected(X, genes, b0, b1, alpha, log_umi, log_umi_ref):
    """-> (c fp64 (n x g): the corrected counts of the listed genes, 0 in every other column; near (n x g) bool: the entries
    within HALF_TOL of a half-integer).  b0, b1, alpha: in the order of ``genes``."""
    X = np.asarray(X)
    genes = np.asarray(genes)
    v = values(X[:, genes], b0, b1, alpha, log_umi, log_umi_ref)
    c, near = np.zeros(X.shape), np.zeros(X.shape, dtype=bool)
    c[:, genes] = count_of(v)
    near[:, genes] = near_half(v)
    return c, near


def data_slot(c):
    """the ``data`` slot of corrected counts c"""
    return np.log1p(c).astype(np.float32)


def reference_depth(log_umi):
    """log10 of the median of the cells' totals"""
    return float(np.log10(np.median(10.0 ** np.asarray(log_umi, dtype=np.float64))))


@functools.lru_cache(maxsize=None)
def inputs(n, g, seed=0):
    """the recipe of tests/test_gpu_sct.py's ``residual_inputs`` (restated, so that the tests off the GPU import no GPU test
    module): counts, log_umi ~ U(2.5, 4), b0 from the column mean, b1 ~ N(2.3, 0.3), alpha 0 for every third gene; and the
    reference depth.  -> (X, log_umi, b0, b1, alpha, log_umi_ref), read-only"""
    rng = np.random.default_rng(1000 * n + g + seed)
    X = ref.sparse_counts(rng, n, g)
    lu = rng.uniform(2.5, 4.0, n)
    b1 = rng.normal(2.3, 0.3, g)
    b0 = np.log(X.astype(np.float64).mean(axis=0) + 0.1) - b1 * lu.mean()
    alpha = np.where(np.arange(g) % 3 == 0, 0.0, rng.uniform(0.0, 1.0, g))
    X[0, 0] = 50000.0
    out = (X, lu, b0, b1, alpha)
    for a in out:
        a.setflags(write=False)
    return out + (reference_depth(lu),)


def listed_genes(g, seed=0):
    """a shuffled subset of about two thirds of the columns (all of them when g = 1)"""
    perm = np.random.default_rng(7000 + g + seed).permutation(g)
    return perm[:max(1, (2 * g + 2) // 3)].astype(np.int32)
