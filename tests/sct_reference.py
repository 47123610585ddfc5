"""The specification of ``preprocess.sctransform``'s device passes, restated in numpy fp64 (scipy's digamma and trigamma):
the gene attributes, the negative-binomial fit of include/mi_prep.h (``mi_prep_nb_fit``) step by step and vectorised over the
genes, the residual moments, the scaled matrix, and the whole driver with the package's host steps (sub-samples,
``sct_regularize``, the eigen-solve).  Test infrastructure: it imports nothing of the package's device path and loads no
library.  Agreement of this chain with R's sctransform / glmGamPoi is unpinned.

``nb_fit`` has three hooks for tests/sct_edge_cases.py, whose defaults leave every result as it was: ``psi`` (another digamma
/ trigamma pair, such as the numpy port of csrc/mi_sct_math.h below), ``nudge`` (a function applied to every result of
``exp``, ``log`` and ``log1p``: one ulp up or down stands in for another libm) and ``trace`` (what each round did)."""
import numpy as np
from scipy.special import digamma, polygamma

import prep_regress_cases as rc
from scrna_seq_qannealing_clustering_amd import preprocess as pp

POISSON_STEPS, MAX_ROUNDS, TOL = 8, 40, 1e-16
RULE_NONE, RULE_NEWTON, RULE_DOUBLE, RULE_HALVE, RULE_QUARTER = 0, 1, 2, 3, 4     # trace["rule"]: what proposed alpha'
CLAMP_NONE, CLAMP_LOW, CLAMP_HIGH = 0, 1, 2                                       # trace["clamp"]: alpha / 8, 8 alpha


def trigamma(x):
    return polygamma(1, x)


SCIPY_PSI = (digamma, trigamma)


def _horner(i2, coefficients):
    s = coefficients[0]
    for c in coefficients[1:]:
        s = c + i2 * s
    return s


def ported_digamma(x):
    """mi_sct::digamma of csrc/mi_sct_math.h in numpy: the same operations in the same order (numpy's log for libm's)"""
    x = np.array(x, dtype=np.float64)
    r = np.zeros_like(x)
    while True:
        low = x < 8.0
        if not low.any():
            break
        r[low] = r[low] - 1.0 / x[low]
        x[low] = x[low] + 1.0
    i = 1.0 / x
    i2 = i * i
    s = _horner(i2, (3617.0 / 8160.0, -1.0 / 12.0, 691.0 / 32760.0, -1.0 / 132.0, 1.0 / 240.0, -1.0 / 252.0, 1.0 / 120.0,
                     -1.0 / 12.0))
    return r + ((np.log(x) - 0.5 * i) + i2 * s)


def ported_trigamma(x):
    """mi_sct::trigamma of csrc/mi_sct_math.h in numpy"""
    x = np.array(x, dtype=np.float64)
    r = np.zeros_like(x)
    while True:
        low = x < 8.0
        if not low.any():
            break
        r[low] = r[low] + 1.0 / (x[low] * x[low])
        x[low] = x[low] + 1.0
    i = 1.0 / x
    i2 = i * i
    s = _horner(i2, (43867.0 / 798.0, -3617.0 / 510.0, 7.0 / 6.0, -691.0 / 2730.0, 5.0 / 66.0, -1.0 / 30.0, 1.0 / 42.0,
                     -1.0 / 30.0, 1.0 / 6.0))
    return r + (i + i2 * (0.5 + i * s))


PORTED_PSI = (ported_digamma, ported_trigamma)


def _same(v):
    return v


def gene_attributes(X):
    """-> detected, log_gmean = log10(expm1(mean log1p x)) per gene"""
    X64 = np.asarray(X, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return (X64 != 0).sum(axis=0), np.log10(np.expm1(np.log1p(X64).sum(axis=0) / X64.shape[0]))


def _solve2(s00, s01, s11, t0, t1):
    det = s00 * s11 - s01 * s01
    return (s11 * t0 - s01 * t1) / det, (s00 * t1 - s01 * t0) / det, det


def alpha_derivatives(Y, mu, alpha, psi=SCIPY_PSI, nudge=None):
    """-> l1, l2: the first and second derivative of the log-likelihood in alpha, per gene (columns of Y, mu)"""
    psi0, psi1 = psi
    nudge = nudge or _same
    th = 1.0 / alpha
    tm = th + mu
    d = Y - mu
    s = ((psi0(Y + th) - psi0(th)) + nudge(np.log1p(-(mu / tm))) - d / tm).sum(axis=0)
    s1 = ((psi1(Y + th) - psi1(th)) + mu / (th * tm) + d / (tm * tm)).sum(axis=0)
    th2 = th * th
    return -(th2 * s), (th2 * th2) * s1 + 2.0 * ((th2 * th) * s)


def score_step(Y, xc, mu, alpha):
    """the Fisher-scoring step of b at `alpha` and `mu` -> d0, d1, U^T I^-1 U, I00, I11, det"""
    den = 1.0 + alpha * mu
    w, u = mu / den, (Y - mu) / den
    x = xc[:, None]
    u0, u1 = u.sum(axis=0), (u * x).sum(axis=0)
    i00, i01, i11 = w.sum(axis=0), (w * x).sum(axis=0), (w * x * x).sum(axis=0)
    d0, d1, det = _solve2(i00, i01, i11, u0, u1)
    return d0, d1, u0 * d0 + u1 * d1, i00, i11, det


def nb_fit(Y, log_umi, max_rounds=MAX_ROUNDS, psi=SCIPY_PSI, nudge=None, trace=False):
    """Y: (m cells, G genes) counts; log_umi: (m,).  -> dict of per-gene arrays, the outputs of mi_prep_nb_fit plus b0c.
    With `trace`, also "trace": per round and gene (max_rounds x G) `ran`, `l2_sign` (-1, 0, 1; 2 for a NaN), `rule` (RULE_*:
    what proposed alpha'; RULE_NONE on a Poisson gene), `clamp` (CLAMP_*: the bound that limited the proposal) and `lam2`."""
    nudge = nudge or _same
    Y = np.asarray(Y, dtype=np.float32).astype(np.float64)
    lu = np.asarray(log_umi, dtype=np.float64)
    m, G = Y.shape
    xmean = lu.sum() / m
    xc = lu - xmean
    x = xc[:, None]
    with np.errstate(all="ignore"):
        # 1. the Poisson start
        mu = Y + 0.1
        eta = nudge(np.log(mu))
        for _ in range(POISSON_STEPS):
            z = eta + (Y - mu) / mu
            wx = mu * x
            b0, b1, _ = _solve2(mu.sum(axis=0), wx.sum(axis=0), (wx * x).sum(axis=0), (mu * z).sum(axis=0), (wx * z).sum(axis=0))
            eta = b0[None, :] + b1[None, :] * x
            mu = nudge(np.exp(eta))
        # 2. the Poisson rule
        d = Y - mu
        T = (d * d - Y).sum(axis=0)
        pois = ~(T > 0)
        alpha = np.where(pois, 0.0, T / (mu * mu).sum(axis=0))
        # 3. the rounds
        iters = np.zeros(G, dtype=np.int32)
        conv = np.zeros(G, dtype=bool)
        se = np.full((3, G), np.nan)
        if trace:
            tr = dict(ran=np.zeros((max_rounds, G), dtype=bool), l2_sign=np.zeros((max_rounds, G), dtype=np.int8),
                      rule=np.zeros((max_rounds, G), dtype=np.int8), clamp=np.zeros((max_rounds, G), dtype=np.int8),
                      lam2=np.full((max_rounds, G), np.nan))
        for rnd in range(max_rounds):
            run = np.flatnonzero(~conv)
            if len(run) == 0:
                break
            Yr, a = Y[:, run], alpha[run]
            mur = nudge(np.exp(b0[run][None, :] + b1[run][None, :] * x))
            p = pois[run]
            l1, l2 = alpha_derivatives(Yr, mur, np.where(p, 1.0, a), psi, nudge)
            anew = np.where(l2 < 0, a - l1 / l2, np.where(l1 > 0, 2.0 * a, 0.5 * a))
            if trace:
                tr["ran"][rnd, run] = True
                tr["l2_sign"][rnd, run] = np.where(np.isnan(l2), 2, np.sign(np.where(np.isnan(l2), 0.0, l2)))
                rule = np.where(l2 < 0, RULE_NEWTON, np.where(l1 > 0, RULE_DOUBLE, RULE_HALVE))
                rule = np.where(anew > 0, rule, RULE_QUARTER)
                tr["rule"][rnd, run] = np.where(p, RULE_NONE, rule)
            anew = np.where(anew > 0, anew, 0.25 * a)
            if trace:
                tr["clamp"][rnd, run] = np.where(p, CLAMP_NONE, np.where(anew < 0.125 * a, CLAMP_LOW,
                                                                         np.where(anew > 8.0 * a, CLAMP_HIGH, CLAMP_NONE)))
            anew = np.where(p, 0.0, np.minimum(np.maximum(anew, 0.125 * a), 8.0 * a))
            d0, d1, lam2, i00, i11, det = score_step(Yr, xc, mur, anew)
            lam2 = np.where(p, lam2, np.where(l2 < 0, lam2 + (l1 * l1) / -l2, np.inf))
            b0[run] += d0
            b1[run] += d1
            alpha[run] = anew
            iters[run] += 1
            conv[run] = lam2 <= TOL
            se[0, run], se[1, run] = np.sqrt(i11 / det), np.sqrt(i00 / det)
            se[2, run] = np.where(~p & (l2 < 0), 1.0 / np.sqrt(np.where(l2 < 0, -l2, 1.0)), np.nan)
            if trace:
                tr["lam2"][rnd, run] = lam2
    out = dict(b0=b0 - b1 * xmean, b0c=b0, b1=b1, alpha=alpha, se_b0c=se[0], se_b1=se[1], se_alpha=se[2], iterations=iters,
               converged=conv, poisson=pois, log_umi_mean=xmean)
    if trace:
        out["trace"] = tr
    return out


def stop_number(Y, log_umi, b0c, b1, alpha, poisson):
    """lambda = the distance to the optimum in standard errors at the given parameters, evaluated directly (no iteration)"""
    Y = np.asarray(Y, dtype=np.float32).astype(np.float64)
    lu = np.asarray(log_umi, dtype=np.float64)
    xc = lu - lu.sum() / len(lu)
    with np.errstate(all="ignore"):
        mu = np.exp(b0c[None, :] + b1[None, :] * xc[:, None])
        l1, l2 = alpha_derivatives(Y, mu, np.where(poisson, 1.0, alpha))
        lam2 = score_step(Y, xc, mu, alpha)[2]
        lam2 = np.where(poisson, lam2, np.where(l2 < 0, lam2 + (l1 * l1) / -l2, np.inf))
    return np.sqrt(np.maximum(lam2, 0.0))


def residuals(X, b0, b1, alpha, log_umi, clip):
    """the clipped Pearson residuals (n x len(b0), fp64) of the columns of X"""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    mu = np.exp(b0[None, :] + b1[None, :] * np.asarray(log_umi)[:, None])
    return np.minimum(np.maximum((X64 - mu) / np.sqrt(mu + alpha[None, :] * (mu * mu)), -clip), clip)


def residual_moments(X, b0, b1, alpha, log_umi, clip):
    r = residuals(X, b0, b1, alpha, log_umi, clip)
    mean = r.sum(axis=0) / r.shape[0]
    return mean, ((r - mean) ** 2).sum(axis=0) / (r.shape[0] - 1)


def scaled_from_stage1(Z1, Q):
    """stages 2 - 5 of mi_prep_sct_select from the stage-1 matrix: -> Z (float32), c, mean, var, flat"""
    c, S = rc.coefficients(Z1, Q)
    mean, ss, var = rc.moments(rc.residuals(Z1, Q, c))
    flat = ss <= rc.FLAT_RTOL * S
    return rc.scaled(Z1, Q, c, mean, np.ones(len(mean)), flat, np.inf), c, mean, var, flat


def sctransform(X, variable_features_n=3000, npcs=50, vars_to_regress=None, ncells=5000, n_genes=2000, min_cells=5, seed=0,
                clip=None):
    """the driver in numpy fp64 -> dict(genes, coords (fp64), Z, loadings, residual_variance, passing, fit, reg)"""
    X = np.asarray(X, dtype=np.float32)
    n = X.shape[0]
    log_umi = np.log10(X.astype(np.float64).sum(axis=1))
    detected, log_gmean = gene_attributes(X)
    passing = np.flatnonzero(detected >= min_cells)
    cells = pp.sct_cell_subsample(n, ncells, seed)
    cand = passing if len(cells) == n else passing[(X[cells] != 0).sum(axis=0)[passing] >= min_cells]
    genes1 = cand[pp.sct_gene_subsample(log_gmean[cand], n_genes, seed)]
    fit = nb_fit(X[np.ix_(cells, genes1)], log_umi[cells])
    reg = pp.sct_regularize(log_gmean[genes1], fit["b0"], fit["b1"], fit["alpha"], log_gmean[passing])
    _, rvar = residual_moments(X[:, passing], reg.b0, reg.b1, reg.alpha, log_umi, np.sqrt(n))
    top = np.argsort(-rvar, kind="stable")[:min(variable_features_n, len(passing))]
    feats = passing[top]
    clip = np.sqrt(n / 30.0) if clip is None else clip
    Z1 = residuals(X[:, feats], reg.b0[top], reg.b1[top], reg.alpha[top], log_umi, clip).astype(np.float32)
    Q = rc.intercept_basis(n) if vars_to_regress is None else pp.design_basis(vars_to_regress, n=n)[0]
    Z = scaled_from_stage1(Z1, Q)[0].astype(np.float64)
    w, V = np.linalg.eigh(Z.T @ Z / (n - 1))
    w, V = w[::-1], V[:, ::-1]
    return dict(genes=feats, coords=Z @ V[:, :npcs], Z=Z, loadings=V[:, :npcs], eigenvalues=w, residual_variance=rvar,
                passing=passing, fit=fit, reg=reg, log_umi=log_umi, genes1=genes1)
