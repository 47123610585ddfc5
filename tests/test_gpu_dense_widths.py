"""The dense chain below 4097 variables at EVERY register width NT = 4 .. 64, on every kernel built for the width, against
the oracle.  GPU only.

The rest of the suite runs dense models of 1 .. 1000 and 2638 variables: NT = 4, 8, 12, 16 and 44.  The cases of
tests/dense_width_cases.py (tests/test_dense_width_cases.py shows without a GPU that every width and ring depth occurs and
that every slot of every model moves on the oracle) run here on K1 (variant 1), K1w with a ring unit of 2 and of 4 rows
(variant 2; also unpaced) and, up to NT = 44, K1m (variant 3): the kernel name asserted, states and accepted counts
bit-equal to oracle/sa_oracle.c, energies to rtol = atol = 1e-9.  Above NT = 44 K1m is refused, from NT = 56 a ring unit of
4 rows asked for by option is refused too (code -5), and the handle serves the next run; without the option the library
takes 2 rows there.  The library's own choice at NT = 48 and 64 (K1w in launches of `chunk_sweeps`, never K1m) and the first
size of K1x beside the last of K1 are pinned as well.

Measured on an MI355X: 11.9 s for the file (53 tests; 1.9 s of it the first test's device start-up), the oracle's runs
included; at most 0.8 s per test after the first."""
import numpy as np
import pytest

import dense_width_cases as dc
from scrna_seq_qannealing_clustering_amd._lib import MiSaError
from scrna_seq_qannealing_clustering_amd.engine import Problem

pytestmark = pytest.mark.gpu


def check(p, ref, what):
    st, en, info = p.fetch()
    assert np.array_equal(st, ref.states), what
    assert info["accepted"] == ref.accepted and info["proposals"] == ref.proposals, what
    assert np.allclose(en, ref.energies, rtol=dc.E_RTOL, atol=1e-9), what


def run(p, n, scenario, variant, unit_rows, pace=1):
    p.set_option("variant", variant)
    p.set_option("unit_rows", unit_rows)
    p.set_option("pace", pace)
    p.anneal(dc.R, dc.BETAS, dc.SEED, **dc.run_kwargs(n, scenario))


@pytest.mark.parametrize("scenario", dc.SCENARIOS)
@pytest.mark.parametrize("n", dc.SIZES)
def test_every_kernel_of_the_width_against_the_oracle(n, scenario):
    ref = dc.reference(n, scenario)
    ran = []
    with Problem.dense(dc.matrix(n)) as p:
        for variant, unit_rows in dc.VARIANTS:
            name = dc.expected(n, variant, unit_rows)
            if name is None:
                continue                                 # (the refusals: test_refusals_leave_the_handle_usable)
            for pace in ((1, 0) if variant == 2 else (1,)):
                run(p, n, scenario, variant, unit_rows, pace)
                assert p.kernel_name() == name and p.launch_count() == 1
                check(p, ref, (name, pace))
            ran.append(name)
    nt = dc.width(n)
    assert len(set(ran)) == len(ran) == 2 + (nt <= 52) + (nt <= dc.MAX_MFMA_NT)


@pytest.mark.parametrize("n", [n for n in dc.SIZES if dc.width(n) >= 48])
def test_refusals_leave_the_handle_usable(n):
    """NT >= 48: K1m is not built; NT >= 56: a ring of 4-row units does not fit into LDS, and asking for one is refused rather
    than served with 2 rows.  The scheduled variant (4) needs K1m for its hot chunks: with fewer than 32 replicas it runs
    as one launch of K1w, with more it is refused.  After every refusal the same handle runs K1, equal to the oracle."""
    nt = dc.width(n)
    ref = dc.reference(n, "init")
    with Problem.dense(dc.matrix(n)) as p:
        def k1_still_runs():
            run(p, n, "init", 1, 0)
            assert p.kernel_name() == dc.expected(n, 1)
            check(p, ref, "K1 after a refusal")

        refused = [(3, 0)] + ([(2, 4)] if nt >= 56 else [])
        for variant, unit_rows in refused:
            assert dc.expected(n, variant, unit_rows) is None
            with pytest.raises(MiSaError) as err:
                run(p, n, "init", variant, unit_rows)
            assert err.value.code == dc.EUNSUPPORTED, err.value
            k1_still_runs()
        # variant 4 with 19 replicas and 5 sweeps: no chunks, so no scheduler and no K1m: K1w on the unit the library picks
        run(p, n, "init", 4, 0)
        assert p.kernel_name() == dc.expected(n, 2, 0) and p.launch_count() == 1
        check(p, ref, "variant 4, one launch")
        # ... and in chunks (32 replicas or more, more sweeps than a chunk): refused, K1m would have to take the first one
        p.set_option("chunk_sweeps", 2)
        with pytest.raises(MiSaError) as err:
            p.anneal(32, dc.BETAS, dc.SEED)
        assert err.value.code == dc.EUNSUPPORTED, err.value
        k1_still_runs()


@pytest.mark.parametrize("n", dc.AUTO_SIZES)
def test_the_librarys_own_choice_above_the_mfma_sizes(n):
    """variant 0 with 40 replicas and 8 sweeps in chunks of 3: K1w in three launches (bits and cached fields stay in HBM
    between them) on a ring unit of 4 rows at NT = 48 and of 2 at NT = 64 -- and never K1m, which is not built there."""
    ref = dc.auto_reference(n)
    with Problem.dense(dc.matrix(n)) as p:
        p.set_option("chunk_sweeps", dc.AUTO_CHUNK)
        p.anneal(dc.AUTO_R, dc.AUTO_BETAS, dc.SEED, replica_offset=dc.REPLICA_OFFSET, resync_interval=dc.AUTO_RESYNC)
        name = p.kernel_name()
        assert name == dc.expected(n, 2, 0) and "mfma" not in name, name
        assert ("dense_wg<48,4>" if n == 2817 else "dense_wg<64,2>") in name
        assert p.launch_count() == 3
        check(p, ref, name)


def test_the_last_size_of_k1_and_the_first_of_k1x():
    """Fresh handles, default options, 3 replicas: 4096 variables run on k_anneal_dense<64>, 4097 on k_anneal_dense_xl<2>."""
    from oracle import sa_oracle as so
    betas = np.geomspace(0.3, 3.0, 3)
    for n, name, rtol, atol in ((4096, "k_anneal_dense<64>", dc.E_RTOL, 1e-9), (4097, "k_anneal_dense_xl<2>", dc.XL_RTOL, dc.XL_ATOL)):
        Qs = dc.matrix(n) if n <= 4096 else dc.xl_model(n)
        ost, oen, ostats = so.sa_dense_philox(Qs, 3, betas, dc.SEED)
        with Problem.dense(Qs) as p:
            p.anneal(3, betas, dc.SEED)
            st, en, info = p.fetch()
            assert p.kernel_name() == name, p.kernel_name()
        assert np.array_equal(st, ost) and info["accepted"] == int(ostats[1]) and info["accepted"] > n
        assert np.allclose(en, oen, rtol=rtol, atol=atol)
