"""The negative-binomial fit on the device (``mi_prep_nb_fit``) where genes stall, fail or sit on a decision edge: the genes of
tests/sct_edge_cases.py at m = 3, 5, 64, 256, 257 and 8192 cells, and the driver with such genes in its step-1 table.
tests/test_gpu_sct.py pins the fit where every gene converges; this file is the rest.

EVERY gene, qualifying or not: two runs give the same bytes (NaN included); a CSR handle that stores some of its zeros gives
the dense handle's bytes; a shuffled ``cells`` / ``genes`` subset of a larger handle gives the bytes of the block uploaded on
its own.

QUALIFYING genes (those the restatement answers firmly under permutation, another psi and another libm: the ensemble of
tests/sct_edge_cases.py, which never sees the device): ``poisson``, ``converged`` and the NaN / inf pattern of the six float
outputs equal the restatement's; ``iterations`` lies in the ensemble's own range widened by one on each side (the +-1 of
tests/test_gpu_sct.py is the case of a zero-width range); ``b0c``, ``b1`` and alpha lie within 100 s + tau() of the
restatement, in the units of s (the gene's own ensemble spread) and with the floor tau() of tests/test_gpu_sct.py; the three
standard errors within max(1e-6, 100 x their relative spread over the ensemble); alpha = 0 and ``se_alpha`` NaN on Poisson
genes.  For a converged gene the stopping number evaluated on the host at the device's parameters lies within the same
100 s + tau(), on the genes where every member of the ensemble meets that bound at its own final iterate (a gene whose
single count sits in the deepest cell does not: its slope runs off, it "converges" in the round before exp overflows, and
the number evaluated afresh at that iterate is NaN in some members).

MEASURED on an MI355X (408 genes, 337 qualifying): all of the above hold.  The largest deviation of a parameter in the
units of s, per class of tests/sct_edge_cases.py: (a) round limit 1.3e-10, (b) failed 4.2e-9, (c) the 8 alpha bound 2.0e-20,
(d) alpha / 8 or the quarter rule 1.3e-10, (e) Poisson constant 4.6e-14, (f) alpha < 1e-3 3.1e-8 (allowed there 1.8e-5), (g) a
count of 2^24 4.2e-9, no class 1.6e-10; the allowance is never below tau() = 2.9e-6.  The stopping number at the device's
parameters is at most 2.1e-7 (class f at 64 cells).  On the excluded genes the device lands inside the ensemble's spread of
outcomes: the run-off gene of the driver's table, NaN in the restatement, ended finite on the device
(``test_edge_fit_matches_the_restatement`` prints each; DESIGN.md section 5c "Edge genes of the fit").  No qualifying gene
has disagreed on the device, so none is recorded here.

The driver: ``preprocess.sctransform(X, cells=..., genes=...)`` on ``sct_cases.planted_counts()`` extended by edge genes, 64
fit cells, 200 planted genes plus the edge genes, dense and CSR, against the chain ``sr.nb_fit`` -> ``pp.sct_regularize`` ->
``sr.residual_moments`` composed here with the same overrides."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import prep_regress_cases as rc
import sct_cases as sc
import sct_edge_cases as ec
import sct_reference as sr
from scrna_seq_qannealing_clustering_amd import preprocess
from scrna_seq_qannealing_clustering_amd.preprocess import ExpressionMatrix
from test_gpu_sct import FIT_KEYS, tau

pytestmark = pytest.mark.gpu


def same_bytes(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in FIT_KEYS)


def csr_with_stored_zeros(Y, rng):
    """-> (dense, csr of it with stored zeros, none of them in an all-zero gene's column).  From four cells on it is
    rc.csr_with_stored_zeros_and_empty_row (which empties cell 3)"""
    if Y.shape[0] > 3:
        X, A = rc.csr_with_stored_zeros_and_empty_row(Y, rng)
        A = A.tocoo()
    else:
        X = Y.copy()
        pattern = (X != 0) | (rng.random(X.shape) < 0.3)
        pattern[tuple(np.argwhere((X == 0) & (Y != 0).any(axis=0)[None, :])[0])] = True
        rows, cols = np.nonzero(pattern)
        A = sp.coo_matrix((X[rows, cols], (rows, cols)), shape=X.shape)
    keep = (Y != 0).any(axis=0)[A.col]                           # (an all-zero gene has no stored entry)
    A = sp.csr_matrix((A.data[keep], (A.row[keep], A.col[keep])), shape=X.shape)
    assert A.nnz > (X != 0).sum()
    return X, A


@functools.lru_cache(maxsize=None)
def device_fits(m):
    """-> the fits of the block of size m: alone (twice), dense and CSR of its stored-zeros form, as a subset of a larger handle"""
    b = ec.block(m)
    Y, lu = b["Y"], b["log_umi"]
    G = Y.shape[1]
    rng = np.random.default_rng(m)
    every_cell, every_gene = np.arange(m), np.arange(G)
    with ExpressionMatrix(Y) as h:
        first, again = h.nb_fit(every_cell, every_gene, lu), h.nb_fit(every_cell, every_gene, lu)
    X2, A = csr_with_stored_zeros(Y, rng)
    with ExpressionMatrix(X2) as d, ExpressionMatrix(A) as s:
        assert s.sparse and not d.sparse
        dense, sparse = d.nb_fit(every_cell, every_gene, lu), s.nb_fit(every_cell, every_gene, lu)
    cells, genes = rng.permutation(m + 37)[:m], rng.permutation(G + 5)[:G]
    big = rng.poisson(2.0, (m + 37, G + 5)).astype(np.float32)
    big[np.ix_(cells, genes)] = Y
    with ExpressionMatrix(big) as h:
        subset = h.nb_fit(cells, genes, lu)
    return dict(first=first, again=again, dense=dense, sparse=sparse, subset=subset)


@pytest.mark.parametrize("m", ec.SIZES)
def test_every_edge_gene_is_reproducible_and_independent_of_the_handle(m):
    f = device_fits(m)
    assert same_bytes(f["first"], f["again"])
    assert same_bytes(f["dense"], f["sparse"])
    assert same_bytes(f["first"], f["subset"])
    assert f["first"].iterations.min() >= 1 and f["first"].iterations.max() <= sr.MAX_ROUNDS


def compare_with_restatement(dev, q, Y, log_umi, use):
    """the assertions on the qualifying genes `use` (a mask); -> worst deviation in the units of s per gene, the stopping
    numbers"""
    fit, t = q["fit"], tau()
    assert t <= 1e-3
    assert np.array_equal(dev.poisson[use], fit["poisson"][use]) and np.array_equal(dev.converged[use], fit["converged"][use])
    for key in ("b0", "b1", "alpha", "se_b0c", "se_b1", "se_alpha"):
        assert np.array_equal(ec.pattern(dev[key])[use], ec.pattern(fit[key])[use]), key
    its = dev.iterations.astype(int)
    assert np.all((its >= q["iterations_lo"] - 1) & (its <= q["iterations_hi"] + 1) | ~use)
    with np.errstate(invalid="ignore"):
        got = dict(b0c=dev.b0 + dev.b1 * dev.log_umi_mean, b1=dev.b1, alpha=dev.alpha)
    bound = 100.0 * q["s"] + t
    worst = np.zeros(len(bound))
    for key, se_key in ec.PARAMETERS:
        dz = ec.deviation(got[key], fit, key, se_key)
        assert np.all((dz <= bound) | ~use), (key, np.flatnonzero((dz > bound) & use), dz[(dz > bound) & use])
        worst = np.maximum(worst, dz)
    for k, key in enumerate(("se_b0c", "se_b1", "se_alpha")):
        rtol = np.maximum(1e-6, 100.0 * q["se_spread"][k])
        with np.errstate(invalid="ignore"):
            off = np.abs(dev[key] - fit[key]) > rtol * np.abs(fit[key])      # (False for a NaN or inf: the pattern is equal)
        assert not (off & use & np.isfinite(fit[key])).any(), (key, np.flatnonzero(off & use))
    p = dev.poisson & use
    assert (dev.alpha[p] == 0).all() and np.isnan(dev.se_alpha[p]).all()
    lam = sr.stop_number(Y, log_umi, got["b0c"], dev.b1, dev.alpha, dev.poisson)
    held = use & fit["converged"] & (q["own_lambda"] <= bound)
    assert np.all((lam <= bound) | ~held), (np.flatnonzero(~(lam <= bound) & held), lam[~(lam <= bound) & held])
    return worst, lam, held


@pytest.mark.parametrize("m", ec.SIZES)
def test_edge_fit_matches_the_restatement(m):
    q = ec.qualified(m)
    dev = device_fits(m)["first"]
    use = q["qualifies"]
    worst, lam, held = compare_with_restatement(dev, q, q["block"]["Y"], q["block"]["log_umi"], use)
    print("m = %d: %d genes, %d excluded; tau %.3g" % (m, len(use), (~use).sum(), tau()))
    for c, text in ec.CLASSES.items():
        sel = q["classes"][c] & use
        if sel.any():
            print("  (%s) %-48s %3d genes: device - restatement %.3g (allowed there %.3g), rounds %d .. %d, lambda %.3g" % (
                c, text, sel.sum(), worst[sel].max(), (100.0 * q["s"] + tau())[sel][np.argmax(worst[sel])],
                dev.iterations[sel].min(), dev.iterations[sel].max(), lam[sel & held].max() if (sel & held).any() else np.nan))
    rest = use & ~np.any([q["classes"][c] for c in ec.CLASSES], axis=0)
    if rest.any():
        print("  (-) %-48s %3d genes: device - restatement %.3g" % ("no class", rest.sum(), worst[rest].max()))
    # what the device does on the genes the restatement does not answer firmly: printed, not asserted
    fit = q["fit"]
    for j in np.flatnonzero(~use):
        print("  excluded gene %d (%s): device rounds %d converged %d poisson %d; restatement %d .. %d converged %d poisson %d"
              % (j, q["block"]["family"][j], dev.iterations[j], dev.converged[j], dev.poisson[j], q["iterations_lo"][j],
                 q["iterations_hi"][j], fit["converged"][j], fit["poisson"][j]))


# ---- the driver ---------------------------------------------------------------------------------------------------------------

N_FIT_CELLS, N_PLANTED_GENES = 64, 200


@functools.lru_cache(maxsize=None)
def driver_case():
    """planted_counts() with edge genes appended (their pattern in the 64 fit cells, a few counts elsewhere so that each has a
    geometric mean), the overrides, and the restated chain"""
    X0, _, _ = sc.planted_counts()
    n = X0.shape[0]
    rng = np.random.default_rng(21)
    cells = np.sort(rng.permutation(n)[:N_FIT_CELLS])
    others = np.setdiff1d(np.arange(n), cells)
    depth = X0.astype(np.float64).sum(axis=1)
    order = cells[np.argsort(depth[cells], kind="stable")]       # the fit cells, shallowest .. deepest
    half = order[N_FIT_CELLS // 2:]
    edge = []

    def add(in_fit, elsewhere):
        y = np.zeros(n)
        y[others] = elsewhere
        for where, value in in_fit:
            y[where] = value
        edge.append(y)

    add([(order[-2], 5000.0)], rng.poisson(0.5, len(others)))    # single non-zero fit cells
    add([(order[1], 7.0)], rng.poisson(0.5, len(others)))
    add([(order[32], 5000.0)], rng.poisson(0.5, len(others)))
    add([(order[20], 1.0)], rng.poisson(0.1, len(others)))
    add([(half, 4.0)], rng.poisson(2.0, len(others)))            # a step in depth and its mirror
    add([(order[:N_FIT_CELLS // 2], 4.0)], rng.poisson(2.0, len(others)))
    add([], rng.poisson(0.3, len(others)))                       # all zero in the fit cells
    add([(cells, 3.0)], np.full(len(others), 3.0))               # constant
    add([(order[[3, 17, 30, 44, 60]], [1.0, 2.0, 300.0, 4.0, 1.0])], rng.poisson(0.2, len(others)))
    X = np.ascontiguousarray(np.column_stack([X0] + edge).astype(np.float32))
    g0 = X0.shape[1]
    edge_genes = np.arange(g0, X.shape[1])
    log_umi = np.log10(X.astype(np.float64).sum(axis=1))
    detected, log_gmean = sr.gene_attributes(X)
    passing = np.flatnonzero(detected >= 5)
    ok = np.flatnonzero((X[cells][:, :g0] != 0).sum(axis=0) >= 5)
    genes = np.concatenate([ok[np.linspace(0, len(ok) - 1, N_PLANTED_GENES).astype(int)], edge_genes])
    Yf = X[np.ix_(cells, genes)]
    q = ec.qualified_block(Yf, log_umi[cells])
    fit = q["fit"]
    reg = preprocess.sct_regularize(log_gmean[genes], fit["b0"], fit["b1"], fit["alpha"], log_gmean[passing])
    _, rvar = sr.residual_moments(X[:, passing], reg.b0, reg.b1, reg.alpha, log_umi, np.sqrt(n))
    feats = passing[np.argsort(-rvar, kind="stable")[:200]]
    X.setflags(write=False)
    return dict(X=X, cells=cells, genes=genes, q=q, reg=reg, feats=feats, passing=passing, is_edge=genes >= g0,
                log_umi=log_umi, Yf=Yf)


@pytest.mark.parametrize("kind", ["dense", "csr"])
def test_driver_with_edge_genes_in_the_step_one_table(kind):
    c = driver_case()
    q, fit, use = c["q"], c["q"]["fit"], c["q"]["qualifies"]
    failed = np.isnan(fit["b0"]) & np.isnan(fit["b1"])
    stalled = ~fit["converged"] & np.isfinite(fit["b0"])
    print("step-1 table: %d genes, %d excluded, %d failed and %d at the round limit among the qualifying"
          % (len(use), (~use).sum(), (failed & use).sum(), (stalled & use).sum()))
    assert failed.any() and (stalled & use).any()                # (the condition of this test; the failed gene runs off)
    X = sp.csr_matrix(c["X"]) if kind == "csr" else c["X"]
    r = preprocess.sctransform(X, variable_features_n=200, npcs=10, cells=c["cells"], genes=c["genes"])
    assert np.array_equal(r.model.genes, c["genes"]) and np.array_equal(r.model.cells, c["cells"])
    assert np.array_equal(r.model.converged[use], fit["converged"][use])
    assert np.array_equal(r.model.poisson[use], fit["poisson"][use])
    compare_with_restatement(r.model, q, c["Yf"], c["log_umi"][c["cells"]], use)
    nonfinite = ~(np.isfinite(r.model.b0) & np.isfinite(r.model.b1) & np.isfinite(r.model.alpha))
    print("device: %d non-finite fits, %d at the round limit, %d outliers" % (nonfinite.sum(), (~r.model.converged).sum(),
                                                                             r.model.outlier.sum()))
    assert r.model.outlier[nonfinite].all() and r.model.outlier[failed].all()
    assert np.array_equal(r.model.outlier[use], c["reg"].outlier[use])
    a = r.gene_attr
    passing = np.flatnonzero(a.passing)
    assert np.array_equal(passing, c["passing"])
    for key in ("b0", "b1", "alpha"):
        assert np.isfinite(a[key][passing]).all(), key
        np.testing.assert_allclose(a[key][passing], c["reg"][key], rtol=1e-6, atol=1e-9)
    assert r.coords.shape == (c["X"].shape[0], 10) and np.isfinite(r.coords).all()
    assert set(r.genes.tolist()) == set(c["feats"].tolist())
