"""k_potts_merge at its edges (tests/potts_merge_cases.py): up to 64 labels, two, three and four passes of 64 proposals,
K = 2, clusters empty from the start, device n of 2, 63, 64, 65 and 257 (unpadded) and their padded layouts, no couplings, rows wider than 64,
holes, node weights at the ABI's limit, resolution groups, per-replica temperatures and a call that opens with a merge
phase.  On every case the device equals the restatement bit for bit on ALL replicas: labels, accepted single-site moves,
accepted merges.  tests/test_potts_merge_cases.py shows that the restatement's runs reach what each case is for."""
import numpy as np
import pytest

import potts_merge_cases as pc
from test_gpu_potts_merge import chain_inputs, problem
from scrna_seq_qannealing_clustering_amd import models

pytestmark = pytest.mark.gpu


def launches_expected(c):
    """One merge launch per merge point of the call and one anneal launch per stretch of sweeps between them:
    2 * len(cuts) + 1, less one when the call opens with a merge phase."""
    cuts = [s for s in range(c.sweep_offset, c.sweep_offset + c.S) if s > 0 and s % c.M == 0]
    return 2 * len(cuts) + 1 - (1 if cuts and cuts[0] == c.sweep_offset else 0)


def same_inputs(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got, want)) and len(got) == len(want)


def device_run(c, pm, sched, rb, start, cq):
    """One single-resolution run of case ``c`` on model ``pm`` -> (labels, energies, accepted, merges, chain inputs)"""
    nw = models.potts_node_weights(pm)
    with problem(pm, order=c.order, weights=nw) as p:
        p.set_merge_moves(c.M, c.P, cq)
        if rb is not None:
            p.anneal(c.R, rb, c.seed, replica_offset=c.replica_offset, initial_states=start, sweep_offset=c.sweep_offset,
                     num_sweeps=c.S)
        else:
            p.anneal(c.R, sched, c.seed, replica_offset=c.replica_offset, initial_states=start,
                     sweep_offset=c.sweep_offset)
        lab, en, info = p.fetch()
        merges = p.merges_accepted()
        assert p.kernel_name() == c.kernel + " + k_potts_merge"
        assert p.launch_count() == launches_expected(c)
        return lab, en, info["accepted"], merges, chain_inputs(p, pm)


def check(c, run, pm, lab, en, accepted, merges, inputs=None):
    ref = pc.reference(run)
    if inputs is not None:
        assert same_inputs(inputs, ref.inputs)                   # the restatement ran on the seats the device uses
    seats = ref.inputs[-1]
    differ = [r for r in range(c.R) if not np.array_equal(lab[r], ref.labels[r, seats])]
    assert not differ, "replicas %s differ from chain 2e" % differ
    assert np.array_equal(lab, ref.labels[:, seats])
    assert accepted == ref.accepted and merges == ref.merges
    assert np.allclose(en, pm.energies(lab), rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("name", [c.name for c in pc.CASES if len(c.gammas) == 1])
def test_device_equals_chain2e_at_the_edges(name):
    c = pc.BY_NAME[name]
    pm = pc.model(name)
    sched, rb = pc.betas(c, pm)
    cq = models.potts_merge_coefficients(pm)
    assert (cq is None) == (c.kind == "dqm")
    for st in c.starts:
        lab, en, accepted, merges, inputs = device_run(c, pm, sched, rb, pc.start_labels(c, st), cq)
        check(c, (name, 0, st), pm, lab, en, accepted, merges, inputs)


@pytest.mark.parametrize("name", [c.name for c in pc.CASES if len(c.gammas) > 1])
def test_groups_equal_chain2e_and_single_runs(name):
    """Resolution groups on the multi-pass path: every group equals the restatement of its own model, and its
    single-resolution run on the device bit for bit."""
    c = pc.BY_NAME[name]
    G = len(c.gammas)
    pms = [pc.model(name, g) for g in range(G)]
    wq, cw, w64, c64, offset = models.potts_node_weight_groups(pms)
    sched = np.stack([pc.betas(c, pm)[0] for pm in pms])
    cqs = models.potts_merge_coefficients(pms)
    with problem(pms[0], order=c.order) as p:
        p.set_node_weight_groups(cw, c64, offset)
        p.set_merge_moves(c.M, c.P, cqs)
        p.anneal(G * c.R, sched, c.seed, replica_offset=c.replica_offset)
        lab, en, info = p.fetch()
        merges = p.merges_accepted()
        assert p.kernel_name() == c.kernel + " + k_potts_merge" and p.launch_count() == launches_expected(c)
        inputs = [chain_inputs(p, pm) for pm in pms]
    tot_acc = tot_m = 0
    for g, pm in enumerate(pms):
        ref = pc.reference((name, g, None))
        rows = slice(g * c.R, (g + 1) * c.R)
        assert same_inputs(inputs[g], ref.inputs)
        assert np.array_equal(lab[rows], ref.labels[:, ref.inputs[-1]])
        assert np.allclose(en[rows], pm.energies(lab[rows]), rtol=1e-9, atol=1e-9)
        l1, e1, a1, m1, _ = device_run(c, pm, sched[g], None, None, cqs[g:g + 1])
        check(c, (name, g, None), pm, l1, e1, a1, m1)
        assert np.array_equal(lab[rows], l1) and np.array_equal(en[rows], e1)
        tot_acc += ref.accepted
        tot_m += ref.merges
    assert info["accepted"] == tot_acc and merges == tot_m
