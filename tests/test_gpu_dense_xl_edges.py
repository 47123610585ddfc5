"""The large-model dense kernels (n > 4096: K1x, and K1g with the fused and the per-block chain) at the edges of their
blocks, groups, column ranges, chunks and replica ranges, against the oracle.  GPU only.

The rest of the suite runs them at n = 4097, 4500, 9000, 17000 and 50000 with 2, 3, 256, 300 and 1024 replicas.  Here
(cases and CPU-side checks: tests/dense_width_cases.py, tests/test_dense_width_cases.py): a last group of 1, 4, 5 and 8
blocks and `ncols` an exact multiple of 256 (B1); the K1x chunk edge 8192 / 8193 (B2); 64, 65, 257, 512 and 513 replicas,
across the default's switch from the fused to the per-block chain (B3); replica ranges that flip nothing, and ranges that
flip in a few blocks of a few groups only -- the `live` masks and the `todo` stream of k_xg_panel, and the first small
pass of a group, which copies F into Tm whether or not anything flipped (B4); a continued run with one temperature per
replica (B5).  States and accepted counts equal the oracle's, energies (from cached fp32 fields) to rtol 1e-5 / atol 1e-3,
K1g's energies to rtol 1e-6 of K1x's; the kernel is asserted in every run.

Measured on an MI355X: 7.9 s for the file (17 tests), the oracle's runs and the models included; at most 2.2 s per test
(the 8192-variable model and the first model of the file), 0.1 - 0.4 s for the others."""
import os

import numpy as np
import pytest

import dense_width_cases as dc
from scrna_seq_qannealing_clustering_amd.engine import Problem

pytestmark = pytest.mark.gpu


def run_form(p, form, name, reps, betas, **kw):
    """One run on (xl_batched, xl_chain) = form; the kernel name must start with ``name``."""
    p.set_option("xl_batched", form[0])
    p.set_option("xl_chain", form[1])
    p.anneal(reps, betas, dc.XL_SEED, **kw)
    st, en, info = p.fetch()
    assert p.kernel_name().startswith(name), (p.kernel_name(), name)
    return st, en, info["accepted"], info["proposals"]


def agree(out, ref, rows=slice(None), what=""):
    """States of ``rows`` equal the oracle's, energies within the bar of cached fp32 fields."""
    assert np.array_equal(out[0][rows], ref.states), what
    assert np.allclose(out[1][rows], ref.energies, rtol=dc.XL_RTOL, atol=dc.XL_ATOL), what


def same_run(outs):
    """K1g (every later entry) against K1x (the first): states and accepted counts equal, energies to rtol 1e-6."""
    for other in outs[1:]:
        assert np.array_equal(other[0], outs[0][0]) and other[2:] == outs[0][2:]
        assert np.allclose(other[1], outs[0][1], rtol=dc.XG_RTOL)


@pytest.mark.parametrize("scenario", dc.SCENARIOS)
@pytest.mark.parametrize("n", dc.B1_SIZES)
def test_group_shapes(n, scenario):
    """B1: a last group of one block, of four (ncols exact), of five with a single variable in the last, and nine full
    groups (ncols exact)."""
    ref = dc.b1_reference(n, scenario)
    kw = dict(replica_offset=dc.XL_OFFSET)
    if scenario == "init":
        kw.update(initial_states=dc.xl_start(n, dc.B1_R), resync_interval=dc.B1_RESYNC)
    outs = []
    with Problem.dense(dc.xl_model(n)) as p:
        for form, name in dc.XL_FORMS:
            if name.startswith("k_x"):
                name += " (K1g, %d blocks of 64 rows in groups of 8)" % dc.xl_shape(n)[0]
            outs.append(run_form(p, form, name, dc.B1_R, dc.B1_BETAS, **kw))
            agree(outs[-1], ref, what=name)
            assert outs[-1][2:] == (ref.accepted, ref.proposals), name
    same_run(outs)
    assert ref.accepted > n


@pytest.mark.parametrize("n", dc.B2_SIZES)
def test_k1x_chunk_edge(n):
    """B2: 8192 variables fill two chunks of 4096 columns, 8193 put one variable into a third."""
    ref = dc.b2_reference(n)
    outs = []
    with Problem.dense(dc.xl_model(n)) as p:
        for form, name in dc.XL_FORMS:
            if form == dc.K1X:
                name = "k_anneal_dense_xl<%d>" % (2 if n == 8192 else 3)
            outs.append(run_form(p, form, name, dc.B2_R, dc.B2_BETAS, replica_offset=dc.XL_OFFSET))
            if form == dc.K1X:
                assert p.kernel_name() == name
            agree(outs[-1], ref, what=name)
            assert outs[-1][2:] == (ref.accepted, ref.proposals), name
    same_run(outs)
    assert ref.accepted > n


@pytest.mark.parametrize("reps", dc.B3_COUNTS)
def test_replica_ranges(reps):
    """B3: one full range of 64 replicas, one replica into the second, into the fifth, 512 (the last count the default
    runs on the fused chain) and 513 (the first on the per-block chain)."""
    n = dc.B3_N
    with Problem.dense(dc.xl_model(n)) as p:
        own = run_form(p, (1, 0), "k_xg_chain" if reps <= 512 else "k_xg_diag", reps, dc.B3_BETAS)
        other = run_form(p, dc.K1G_BLOCK if reps <= 512 else dc.K1G_FUSED, "k_xg_diag" if reps <= 512 else "k_xg_chain",
                         reps, dc.B3_BETAS)
        k1x = run_form(p, dc.K1X, "k_anneal_dense_xl<2>", reps, dc.B3_BETAS)
    same_run([k1x, own, other])
    assert own[3] == reps * len(dc.B3_BETAS) * n and own[2] > reps * n // 2
    for lo, count in dc.b3_windows(reps):
        ref = dc.b3_reference(lo, count)
        for out in (k1x, own, other):
            agree(out, ref, rows=slice(lo, lo + count), what=(lo, count))


def test_dead_and_partly_live_ranges():
    """B4: 192 replicas, one temperature each.  The first range of 64 is hot and flips everywhere; the second starts from
    all zeros at beta = 1e4 and flips nothing in any sweep; the third, as cold, starts from all zeros but a few planted
    ones, which flip back in the first sweep: it is live in blocks 1 and 6 of group 1, block 0 of group 2, the last block
    of group 3 and the last block (one variable) of the last group, and nowhere else."""
    n = dc.B4_N
    betas, init = dc.b4_inputs()
    ref = dc.b4_reference()
    planted = len(dc.b4_planted())
    forms = dc.XL_FORMS + ((dc.K1G_FUSED, "k_xg_chain + k_xg_panel"), (dc.K1G_BLOCK, "k_xg_diag + k_xg_panel"))
    outs = []
    with Problem.dense(dc.xl_model(n)) as p:
        for i, (form, name) in enumerate(forms):
            one_stream = i >= len(dc.XL_FORMS)                       # the last two: K1g's kernels in the caller's stream
            if one_stream:
                os.environ["MI_XG_ONE_STREAM"] = "1"
            try:
                outs.append(run_form(p, form, name, dc.B4_R, betas, initial_states=init, num_sweeps=dc.B4_SWEEPS))
                # the cold third alone: exactly the planted ones move, whatever the oracle says
                alone = run_form(p, form, name, 64, betas[128:], initial_states=init[128:], num_sweeps=dc.B4_SWEEPS,
                                 replica_offset=128)
            finally:
                if one_stream:
                    del os.environ["MI_XG_ONE_STREAM"]
            what = (name, "one stream" if one_stream else "")
            agree(outs[-1], ref, what=what)
            assert outs[-1][2:] == (ref.accepted, ref.proposals), what
            assert not outs[-1][0][64:].any(), what
            assert alone[2] == planted and not alone[0].any(), what
            assert np.allclose(alone[1], 0.0, atol=dc.XL_ATOL), what
    same_run(outs)


def test_continued_run_with_one_temperature_per_replica():
    """B5: two sweeps, then two more from the states on the device with the random stream of sweep 2 onwards and one
    constant temperature per replica, against the oracle continued the same way."""
    n = dc.B5_N
    first, then = dc.b5_reference()
    outs = []
    with Problem.dense(dc.xl_model(n)) as p:
        for form, name in dc.XL_FORMS:
            a = run_form(p, form, name, dc.B5_R, dc.B5_BETAS, replica_offset=dc.XL_OFFSET)
            agree(a, first, what=name)
            assert a[2:] == (first.accepted, first.proposals)
            outs.append(run_form(p, form, name, dc.B5_R, dc.B5_RUNG, replica_offset=dc.XL_OFFSET, num_sweeps=2, sweep_offset=2,
                                 continue_run=True))
            agree(outs[-1], then, what=name)
            assert outs[-1][2:] == (then.accepted, then.proposals), name
    same_run(outs)
    assert then.accepted > dc.B5_R * n // 2 and not np.array_equal(first.states, then.states)
