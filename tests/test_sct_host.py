"""SCTransform off the GPU: the specification (tests/sct_reference.py, numpy fp64) converges on the test inputs and recovers
the planted parameters; the host steps of ``preprocess`` (sub-samples, ``bw_sj``, ``kernel_smooth``, ``sct_regularize``) do
what they say; the device's digamma and trigamma, compiled as a host program, agree with scipy; and the whole chain on the
restatement finds planted markers, leaves null genes at unit residual variance and takes sequencing depth out of the PCs."""
import math
import os
import subprocess

import numpy as np
import pytest
from numpy.polynomial.hermite_e import hermeval
from scipy.special import digamma, polygamma

import prep_reference as ref
import prep_regress_cases as rc
import sct_cases as sc
import sct_reference as sr
from scrna_seq_qannealing_clustering_amd import preprocess as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", sc.FIT_CASES)
def test_every_gene_converges_within_the_round_limit(case):
    d = sc.nb_counts(*case)
    f = sr.nb_fit(d["Y"], d["log_umi"])
    assert f["converged"].all() and f["iterations"].max() <= sr.MAX_ROUNDS
    assert np.isfinite(f["se_alpha"][~f["poisson"]]).all()       # (no gene ends where the likelihood is not concave in alpha)
    assert (f["alpha"][f["poisson"]] == 0).all() and (f["alpha"][~f["poisson"]] > 0).all()


def test_fit_recovers_the_planted_parameters():
    d = sc.nb_counts(*sc.FIT_CASES[0])
    sc.check_recovery(sr.nb_fit(d["Y"], d["log_umi"]), d)


def test_bw_sj_satisfies_its_defining_equation():
    """SD and TD here are the full n x n sums of the 4th and 6th derivative of the normal density, written with numpy's
    Hermite polynomials: another expression than bw_sj's upper-triangle sums"""
    x = np.random.default_rng(5).normal(size=300) * np.array([1.0, 0.3])[np.arange(300) % 2] + (np.arange(300) % 2)
    h = pp.bw_sj(x)
    n = len(x)
    q75, q25 = np.percentile(x, [75, 25])
    scale = min(x.std(ddof=1), (q75 - q25) / 1.349)

    def functional(order, width):
        u = (x[:, None] - x[None, :]) / width
        c = np.zeros(order + 1)
        c[order] = 1.0
        return (hermeval(u, c) * np.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)).sum() / (n * (n - 1) * width ** (order + 1))

    alph2 = 1.357 * (functional(4, 1.24 * scale * n ** (-1 / 7)) / -functional(6, 1.23 * scale * n ** (-1 / 9))) ** (1 / 7)
    rhs = (1.0 / (2.0 * math.sqrt(math.pi) * n * functional(4, alph2 * h ** (5 / 7)))) ** 0.2
    assert 0.05 < h < 0.5
    assert abs(rhs - h) <= 1e-8 * h                               # (bisection to 1e-10 of h; the slope of rhs - h is O(1))


def test_kernel_smooth_equals_a_direct_double_loop():
    rng = np.random.default_rng(6)
    x, y, xo, bw = rng.uniform(0, 3, 40), rng.normal(size=(40, 2)), rng.uniform(-0.5, 3.5, 25), 0.8
    sd = 0.3706506 * bw
    want = np.full((25, 2), np.nan)
    for a in range(25):
        num, den = np.zeros(2), 0.0
        for b in range(40):
            if abs(xo[a] - x[b]) <= 4 * sd:
                w = math.exp(-0.5 * ((xo[a] - x[b]) / sd) ** 2)
                num, den = num + w * y[b], den + w
        if den > 0:
            want[a] = num / den
    got = pp.kernel_smooth(x, y, xo, bw)
    assert np.allclose(got, want, rtol=1e-13, atol=0, equal_nan=True)
    assert np.allclose(pp.kernel_smooth(x, y[:, 0], xo, bw), got[:, 0], rtol=1e-13, atol=0, equal_nan=True)
    # the kernel's quartiles sit at +- bw / 4 (R's ksmooth): Phi(0.25 bw / sd) = 0.75
    assert abs(0.5 * (1 + math.erf(0.25 * bw / sd / math.sqrt(2))) - 0.75) < 1e-7


def test_regularize_reproduces_a_smooth_planted_curve():
    """On an even grid a point further than 4 sd from both ends has symmetric weights, so the linear term of the curve
    cancels and |smooth - f| <= max |f''| / 2 * sum w d^2 / sum w <= max |f''| sd^2 / 2 (the second moment of a truncated
    normal is below sd^2; the grid is 30 points per sd)."""
    x = np.linspace(-2.0, 1.0, 401)
    curves = (lambda t: 1.0 + 0.8 * t + 0.3 * t * t, lambda t: 2.3 + 0.2 * np.sin(1.5 * t), lambda t: 0.4 + 0.1 * t + 0.05 * t * t)
    second = (0.6, 0.2 * 1.5 ** 2, 0.1)
    b0, b1, od = (f(x) for f in curves)
    reg = pp.sct_regularize(x, b0, b1, (10.0 ** od - 1.0) / 10.0 ** x, x)
    assert not reg.outlier.any()
    sd = 0.3706506 * reg.bandwidth
    inner = (x > x[0] + 4 * sd) & (x < x[-1] - 4 * sd)
    assert inner.sum() > 50 and reg.bandwidth == 3.0 * pp.bw_sj(x)
    for got, want, f2 in zip((reg.b0, reg.b1, reg.od), (b0, b1, od), second):
        assert np.abs(got - want)[inner].max() <= 0.5 * f2 * sd * sd * (1 + 1e-6) + 1e-12
        assert np.abs(got - want)[inner].max() > 1e-6             # (it is a smoother, not an interpolation)
    assert np.allclose(reg.alpha, (10.0 ** reg.od - 1.0) / 10.0 ** x, rtol=1e-12)
    # evaluation outside the fitted range is clamped to its ends
    out = pp.sct_regularize(x, b0, b1, (10.0 ** od - 1.0) / 10.0 ** x, np.array([-5.0, 4.0]))
    assert out.b0[0] == reg.b0[0] and out.b0[1] == reg.b0[-1]


def test_regularize_drops_an_outlier_and_a_failed_fit():
    rng = np.random.default_rng(7)
    x = np.sort(rng.uniform(-2, 1, 300))
    b0, b1, alpha = 1 + x + rng.normal(0, 0.05, 300), 2.3 + rng.normal(0, 0.05, 300), 0.2 + rng.uniform(0, 0.02, 300)
    b1[100] += 5.0
    b0[200] = np.nan
    reg = pp.sct_regularize(x, b0, b1, alpha, x)
    assert reg.outlier[100] and reg.outlier[200] and reg.outlier.sum() <= 5
    assert np.abs(reg.b1 - 2.3).max() < 0.05


def test_subsamples_are_deterministic_sorted_and_distinct():
    assert np.array_equal(pp.sct_cell_subsample(40, 50), np.arange(40))
    a, b, c = pp.sct_cell_subsample(1000, 100, seed=3), pp.sct_cell_subsample(1000, 100, seed=3), pp.sct_cell_subsample(1000, 100, 4)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert len(a) == 100 and (np.diff(a) > 0).all() and a.min() >= 0 and a.max() < 1000
    x = np.concatenate([np.random.default_rng(8).normal(0, 0.1, 900), np.linspace(2, 3, 100)])
    assert np.array_equal(pp.sct_gene_subsample(x[:50], 60), np.arange(50))
    g1, g2 = pp.sct_gene_subsample(x, 200, seed=1), pp.sct_gene_subsample(x, 200, seed=1)
    assert np.array_equal(g1, g2) and len(g1) == 200 and (np.diff(g1) > 0).all() and g1.max() < 1000
    assert (g1 >= 900).sum() > 60                                 # the thin tail (10 % of the genes) is drawn far above its share


def test_device_psi_functions_as_a_host_program_agree_with_scipy(tmp_path):
    """The grid is [1e-30, 1e30]: the fit calls both functions at theta = 1 / alpha and at y + theta, and on the genes of
    tests/sct_edge_cases.py the arguments run from 1.1e-20 (an all-zero gene, whose alpha rides the 8 alpha bound to 1e20)
    to 2.4e22 (a nearly Poisson gene whose alpha halves round after round); eight more decades on either side cost nothing.
    Both bounds are relative, 32 roundings; the digamma's is relative to max(1, |psi|), that is absolute about its root at
    1.4616, where the value vanishes and a relative bound means nothing (the fit takes differences of digammas, so the
    absolute error is what it sees); the root's neighbourhood is asserted on its own as well.  MEASURED on this grid:
    trigamma within 9.3e-16 relative, digamma within 8.9e-16 max(1, |psi|) and 4.6e-16 absolute within 0.05 of the root."""
    exe = str(tmp_path / "sct_psi")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "host", "sct_psi_main.cpp")], check=True)
    out = subprocess.run([exe, "12001"], capture_output=True, text=True, check=True).stdout
    a = np.array([[float.fromhex(t) for t in line.split()] for line in out.splitlines()])
    x = a[:, 0]
    assert len(x) == 12001 and abs(x[0] - 1e-30) < 1e-43 and abs(x[-1] - 1e30) < 1e17
    psi, tri = digamma(x), polygamma(1, x)
    bound = 32 * 2.0 ** -53
    assert (np.abs(a[:, 1] - psi) <= bound * np.maximum(1.0, np.abs(psi))).all()
    assert (np.abs(a[:, 2] - tri) <= bound * tri).all()
    near_root = np.abs(x - 1.4616321449683623) < 0.05
    assert near_root.sum() >= 5 and (np.abs(a[near_root, 1] - psi[near_root]) <= bound).all()
    print("digamma: %.3g of max(1, |psi|), %.3g absolute near the root; trigamma: %.3g relative" % (
        (np.abs(a[:, 1] - psi) / np.maximum(1.0, np.abs(psi))).max(), np.abs(a[near_root, 1] - psi[near_root]).max(),
        (np.abs(a[:, 2] - tri) / tri).max()))


@pytest.fixture(scope="module")
def planted_chain():
    X, groups, marker = sc.planted_counts()
    return X, groups, marker, sr.sctransform(X, variable_features_n=200, npcs=10)


def test_restated_chain_ranks_every_marker_among_the_top_200(planted_chain):
    X, _, marker, r = planted_chain
    rv = np.full(X.shape[1], -1.0)
    rv[r["passing"]] = r["residual_variance"]
    top = np.argsort(-rv, kind="stable")[:200]
    assert np.isin(np.flatnonzero(marker), top).all()
    assert r["fit"]["converged"].all()


def test_restated_chain_leaves_null_genes_at_unit_residual_variance(planted_chain):
    X, _, marker, r = planted_chain
    null = ~marker[r["passing"]]
    assert 0.8 <= np.median(r["residual_variance"][null]) <= 1.25


def test_restated_chain_takes_depth_out_of_the_leading_pcs(planted_chain):
    X, _, _, r = planted_chain
    coords, _, _ = ref.pca_coords(X, 200, 10, pp.loess_fit)
    assert rc.max_abs_corr(r["coords"][:, :5], r["log_umi"]).max() < rc.max_abs_corr(coords[:, :5], r["log_umi"]).max()
