"""Inputs of the SCTransform tests (tests/test_sct_host.py, tests/test_gpu_sct.py): gamma-Poisson counts with planted
regression parameters, and counts with planted groups of cells for the end-to-end checks."""
import functools
import math

import numpy as np

FIT_CASES = ((600, 256, 1), (257, 130, 2), (64, 130, 4))         # (cells, genes drawn, seed)


@functools.lru_cache(maxsize=None)
def nb_counts(m, G, seed, min_cells=5):
    """depth log-normal (median 2000, sigma 0.5); gene base means 10^U(-2.3, 1.5) at the median depth; slopes N(2.3, 0.3) on
    log10 depth (natural-log coefficient); theta = 10^U(-0.5, 2), every 7th gene Poisson; counts gamma-Poisson; genes detected
    in fewer than `min_cells` cells dropped.  -> dict(Y (m x G', float32), log_umi (of the drawn depth), alpha, b1, poisson)"""
    rng = np.random.default_rng(seed)
    depth = 2000.0 * np.exp(rng.normal(0.0, 0.5, m))
    base = 10.0 ** rng.uniform(-2.3, 1.5, G)
    slope = rng.normal(2.3, 0.3, G)
    theta = 10.0 ** rng.uniform(-0.5, 2.0, G)
    pois = np.arange(G) % 7 == 0
    lu = np.log10(depth)
    mu = base[None, :] * np.exp(slope[None, :] * (lu - np.log10(2000.0))[:, None])
    lam = np.where(pois[None, :], mu, rng.gamma(theta[None, :], mu / theta[None, :], (m, G)))
    Y = rng.poisson(lam).astype(np.float32)
    keep = (Y != 0).sum(axis=0) >= min_cells
    out = dict(Y=np.ascontiguousarray(Y[:, keep]), log_umi=lu, alpha=np.where(pois, 0.0, 1.0 / theta)[keep], b1=slope[keep],
               poisson=pois[keep])
    for a in out.values():
        a.setflags(write=False)
    return out


PLANTED = dict(n=450, g=900, groups=3, markers=40, fold=8.0, theta=5.0)


@functools.lru_cache(maxsize=None)
def planted_counts(seed=3):
    """three groups of cells (shuffled, equal sizes), genes 40 c .. 40 c + 39 at `fold` times their base rate in group c,
    mean counts 10^U(-1, 1) per gene at the median depth, depth 10-fold (10^U(-0.5, 0.5)) times 3000, gamma-Poisson with theta = 5.
    -> (counts float32 (n x g), groups, marker mask)"""
    p = PLANTED
    rng = np.random.default_rng(seed)
    groups = rng.permutation(np.arange(p["n"]) % p["groups"])
    base = 10.0 ** rng.uniform(-1.0, 1.0, p["g"]) / 3000.0
    depth = 3000.0 * 10.0 ** rng.uniform(-0.5, 0.5, p["n"])
    rate = np.tile(base, (p["n"], 1))
    for c in range(p["groups"]):
        rate[np.ix_(groups == c, np.arange(p["markers"] * c, p["markers"] * (c + 1)))] *= p["fold"]
    mu = rate * depth[:, None]
    X = rng.poisson(rng.gamma(p["theta"], mu / p["theta"])).astype(np.float32)
    marker = np.arange(p["g"]) < p["groups"] * p["markers"]
    X.setflags(write=False)
    return X, groups, marker


def planted_covariate(seed=99):
    """a per-cell technical covariate drawn independently of the groups (a share of counts in some of the genes would not
    be: the first genes are the markers, and every share moves with the group's total)"""
    return np.random.default_rng(seed).normal(size=PLANTED["n"])


def check_recovery(fit, planted):
    """z = (estimate - truth) / se over the genes: |mean z| <= 4 / sqrt(G), 0.6 <= sd z <= 1.4"""
    use = ~np.asarray(fit["poisson"]) & ~planted["poisson"]
    for z in ((fit["alpha"] - planted["alpha"])[use] / fit["se_alpha"][use], (fit["b1"] - planted["b1"]) / fit["se_b1"]):
        assert abs(z.mean()) <= 4.0 / math.sqrt(len(z)), z.mean()
        assert 0.6 <= z.std(ddof=1) <= 1.4, z.std(ddof=1)
    assert use.sum() >= 100
