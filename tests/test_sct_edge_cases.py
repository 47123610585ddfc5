"""The conditions that keep tests/test_gpu_sct_edges.py honest, checked off the GPU on the restatement alone: the hooks of
``sr.nb_fit`` leave its results as they were, the numpy port of the device's psi functions is those functions, few genes of
tests/sct_edge_cases.py are excluded as ill-posed, and every outcome the kernel's control flow can reach -- the round limit, a
failed fit, either bound of the alpha step, the Poisson rule on a constant gene, a nearly Poisson gene, a count of 2^24 --
is reached by at least three genes that qualify."""
import numpy as np
import pytest
from scipy.special import digamma, polygamma

import sct_cases as sc
import sct_edge_cases as ec
import sct_reference as sr


def test_hooks_at_their_defaults_change_no_bit():
    d = sc.nb_counts(*sc.FIT_CASES[2])
    plain = sr.nb_fit(d["Y"], d["log_umi"])
    hooked = sr.nb_fit(d["Y"], d["log_umi"], psi=(digamma, lambda x: polygamma(1, x)), nudge=lambda v: v, trace=True)
    for key, want in plain.items():
        assert np.asarray(hooked[key]).tobytes() == np.asarray(want).tobytes(), key
    tr = hooked["trace"]
    assert np.array_equal(tr["ran"].sum(axis=0), plain["iterations"])
    assert (tr["rule"][tr["ran"] & plain["poisson"][None, :]] == sr.RULE_NONE).all()
    assert (tr["rule"][tr["ran"] & ~plain["poisson"][None, :]] != sr.RULE_NONE).all()
    last = tr["lam2"][plain["iterations"] - 1, np.arange(len(plain["b1"]))]
    assert (last <= sr.TOL).all() and plain["converged"].all()
    # the perturbations move a well-posed gene by far less than a standard error, and do move it
    for kw in (dict(psi=sr.PORTED_PSI), dict(nudge=ec.nudge_up), dict(nudge=ec.nudge_down)):
        other = sr.nb_fit(d["Y"], d["log_umi"], **kw)
        dz = np.abs(other["b1"] - plain["b1"]) / plain["se_b1"]
        assert 0 < dz.max() <= 1e-6, (kw, dz.max())


def test_the_ported_psi_functions_agree_with_scipy():
    """the same bound as the host program's (tests/test_sct_host.py): 32 roundings, the digamma's relative to max(1, |psi|)"""
    x = 10.0 ** np.linspace(-30.0, 30.0, 6001)
    psi, tri = digamma(x), polygamma(1, x)
    bound = 32 * 2.0 ** -53
    assert (np.abs(sr.ported_digamma(x) - psi) <= bound * np.maximum(1.0, np.abs(psi))).all()
    assert (np.abs(sr.ported_trigamma(x) - tri) <= bound * tri).all()


def test_blocks_have_the_sizes_and_families_of_the_kernel_edges():
    families = {"single", "few_large", "step", "constant", "poisson", "under_dispersed", "gamma_poisson", "large"}
    for m in ec.SIZES:
        b = ec.block(m)
        assert b["Y"].shape[0] == m == len(b["log_umi"]) and b["Y"].dtype == np.float32
        assert set(b["family"].tolist()) == families
        assert (b["Y"][:, b["family"] == "constant"] == 0).all(axis=0).sum() == 1                  # the all-zero gene
        assert (b["Y"] >= ec.TWO24).any() and (b["Y"] >= 0).all() and np.isfinite(b["Y"]).all()
        assert np.array_equal(b["Y"], ec.block.__wrapped__(m)["Y"])          # seeded
    assert ec.block(8192)["Y"].shape[1] <= 8
    assert all(np.unique(ec.block(m)["family"], return_counts=True)[1].min() >= 4 for m in ec.SIZES[:-1])


@pytest.mark.parametrize("m", ec.SIZES)
def test_at_most_a_quarter_of_a_family_is_excluded_at_any_size(m):
    """(the ensemble of a size runs once, here, and is shared with the tests below)"""
    q = ec.qualified(m)
    fam, keep = q["block"]["family"], ~ec.runs_off(q["block"]["Y"], q["block"]["log_umi"])
    for f in np.unique(fam):
        assert (~q["qualifies"][(fam == f) & keep]).mean() <= 0.25, (f, m)


def test_few_genes_are_excluded_and_every_outcome_class_qualifies():
    """The shares are over the genes that have an optimum to be compared at.  A gene whose only count sits in the deepest or
    the shallowest cell has none (``ec.runs_off``): it ends converged or failed by rounding, the ensemble excludes nearly
    every one of them at every size (2 of 3 single-cell genes at m = 3, where the issue's 25 % cannot hold for them), and
    their own count is printed.  MEASURED: 7 of 338 other genes excluded (2.1 %), at worst 2 of the 8 large-count genes at
    m = 257 (a Poisson gene at 1e5 counts, whose stopping number has a rounding floor near 1e-12 and whose round count
    therefore runs from 5 to 40 over the ensemble); 56 of the 62 genes that run off excluded; qualifying genes per class
    (a) 74, (b) 6, (c) 18, (d) 5, (e) 17, (f) 9, (g) 15."""
    shares, overall, per_class = ec.report()
    assert max(shares.values()) <= 0.25, {k: v for k, v in shares.items() if v > 0.25}
    assert overall <= 0.10
    assert min(per_class.values()) >= 3, per_class
    failed = sum(int((ec.qualified(m)["classes"]["b"] & ec.qualified(m)["qualifies"]).sum()) for m in ec.SIZES if m <= 64)
    assert failed >= 3, failed


def test_genes_that_run_off_are_the_single_counts_in_an_extreme_cell():
    lu = np.array([3.0, 3.5, 2.5, 3.2])
    Y = np.array([[0, 0, 2, 1], [5, 0, 0, 1], [0, 7, 0, 0], [0, 0, 0, 0]], dtype=np.float32)
    assert ec.runs_off(Y, lu).tolist() == [True, True, False, False]        # deepest, shallowest, interior, two cells
    assert not ec.runs_off(np.zeros((4, 1), dtype=np.float32), lu).any()


def test_a_qualifying_gene_holds_under_a_perturbation_outside_the_ensemble():
    """a permutation, the ported psi pair and a random nudge together, none of them a member: every qualifying gene keeps
    its flags and its NaN pattern and stays within 100 s + 1e-8 standard errors -- the bound the device is held to, with a
    floor below its tau()"""
    for m in ec.SIZES[:-1]:
        q = ec.qualified(m)
        b, fit, use = q["block"], q["fit"], q["qualifies"]
        perm = np.random.default_rng(999).permutation(m)
        other = sr.nb_fit(b["Y"][perm], b["log_umi"][perm], psi=sr.PORTED_PSI, nudge=ec.random_nudge(998))
        for key in ("poisson", "converged"):
            assert np.array_equal(other[key][use], fit[key][use]), (m, key)
        for key in ec.FLOATS:
            assert np.array_equal(ec.pattern(other[key])[use], ec.pattern(fit[key])[use]), (m, key)
        for key, se_key in ec.PARAMETERS:
            dz = ec.deviation(other[key], fit, key, se_key)
            assert np.all((dz <= 100.0 * q["s"] + 1e-8) | ~use), (m, key, np.flatnonzero((dz > 100.0 * q["s"] + 1e-8) & use))
