"""Merge moves on the GPU (chain 2e, mi_sa_problem_set_merge_moves, k_potts_merge): the device equals the test-side
restatement bit for bit (labels, accepted single-site moves, accepted merges) on K3f with and without its threshold
wavefront and on K3, for modularity and unweighted DQM models, merge intervals that do and do not divide the sweep
count, per-replica temperatures and resolution groups; a run continued across a merge boundary equals one call;
interval 0 is the chain without merges; the C ABI's errors; and the modularity driver with merges reaches networkx
Louvain's modularity in a quarter of its default sweeps."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_modularity import bench, device_model, graph, problem
from test_potts_merge_model import chain2e
from scrna_seq_qannealing_clustering_amd import _lib, models
from scrna_seq_qannealing_clustering_amd.engine import Problem
from scrna_seq_qannealing_clustering_amd.sampler import default_potts_beta_range

pytestmark = pytest.mark.gpu

LOUVAIN_Q = 0.8229          # networkx Louvain on the bench graph at resolution 1, seed 0


def model_of(name, kind, K, gamma=1.0):
    G = graph(name)
    return models.build_modularity_potts(G, gamma, K) if kind == "mod" else models.build_dqm_potts(G, K, 0.005)


def chain_inputs(p, pm):
    """(rowptr, col, val, wq, cw, cq, absent, seats) of the model as the device sweeps it."""
    nw = models.potts_node_weights(pm)
    if nw is None:
        c32 = np.float32(pm.c_pair)
        wq, cw, cq = np.ones(pm.num_variables, dtype=np.int64), np.full(pm.num_variables, c32), float(c32)
    else:
        wq, cw, cq = nw[0], nw[1], float(models.potts_merge_coefficients(pm)[0])
    rp, cc, vv, dq, dc, absent, seats = device_model(p, pm, wq, cw)
    return rp, cc, vv, dq, dc, cq, absent, seats


# ---- 1. device = chain 2e -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,kind,K,R,k3,M,S,per_replica,kernel", [
    ("s16", "mod", 12, 1100, 0, 5, 12, False, "k_anneal_potts_fast<16, 16, weighted>"),
    ("s32", "mod", 16, 1100, 0, 4, 9, False, "k_anneal_potts_fast<32, 16, weighted>"),
    ("s16", "mod", 8, 64, 0, 1, 6, False, "k_anneal_potts_fast<16, 8, tw, weighted>"),
    ("s32", "mod", 12, 12, 0, 5, 12, True, "k_anneal_potts_fast<32, 16, tw, weighted>"),
    ("s16", "dqm", 8, 12, 0, 4, 12, False, "k_anneal_potts_fast<16, 8, tw>"),
    ("s32", "dqm", 24, 12, 2, 7, 12, False, "k_anneal_potts<32>"),
    ("s32", "mod", 24, 12, 2, 5, 12, False, "k_anneal_potts<32, weighted>"),
    ("s16", "mod", 24, 12, 2, 3, 10, True, "k_anneal_potts<16, weighted>"),
])
def test_device_equals_chain2e(name, kind, K, R, k3, M, S, per_replica, kernel):
    pm = model_of(name, kind, K)
    lo, hi = default_potts_beta_range(pm)
    hot = lo * 4.0                                           # (a schedule on which merges are accepted)
    betas = models.make_beta_schedule(S, (hot, hi))
    P, seed, ro = 2 * K + 3, 29, 5
    with problem(pm) as p:
        if k3:
            p.set_option("k3_fast", k3)
        nw = models.potts_node_weights(pm)
        p.set_merge_moves(M, P, None if nw is None else models.potts_merge_coefficients(pm))
        if per_replica:
            rb = np.geomspace(hot, hi, R)
            p.anneal(R, rb, seed, replica_offset=ro, num_sweeps=S)
        else:
            p.anneal(R, betas, seed, replica_offset=ro)
        lab, en, info = p.fetch()
        merges = p.merges_accepted()
        assert p.kernel_name() == kernel + " + k_potts_merge"
        cuts = [s for s in range(1, S) if s % M == 0]
        assert p.launch_count() == 2 * len(cuts) + 1
        rp, cc, vv, dq, dc, cq, absent, seats = chain_inputs(p, pm)
    pick = [0, 7] if R > 64 else list(range(R))
    olab, oacc, omerges = chain2e(rp, cc, vv, dq, dc, cq, K, R, betas, seed, M, P, replica_offset=ro, absent=absent,
                                  replicas=pick, per_replica=rb if per_replica else None)
    assert np.array_equal(lab[pick], olab[:, seats])
    if R <= 64:
        assert info["accepted"] == oacc and merges == omerges
    assert merges > 0 and info["accepted"] > 0
    assert np.allclose(en, pm.energies(lab), rtol=1e-9, atol=1e-9)


# ---- 2. resolution groups: group g = its single-resolution merged run -----------------------------------------------

@pytest.mark.parametrize("name,K,Rg", [("s16", 12, 6), ("s32", 8, 400)])
def test_groups_equal_single_runs(name, K, Rg):
    gammas = (0.5, 1.0, 1.6)
    pms = models.build_modularity_sweep(graph(name), gammas, K)
    wq, cw, w64, c64, offset = models.potts_node_weight_groups(pms)
    S, M, P = 12, 5, 20
    betas = np.stack([models.make_beta_schedule(S, (4.0 * default_potts_beta_range(pm)[0],
                                                    default_potts_beta_range(pm)[1])) for pm in pms])
    cqs = models.potts_merge_coefficients(pms)
    with problem(pms[0]) as p:
        p.set_node_weight_groups(cw, c64, offset)
        p.set_merge_moves(M, P, cqs)
        p.anneal(3 * Rg, betas, 41, replica_offset=2)
        lab, en, info = p.fetch()
        merges = p.merges_accepted()
    tot_acc = tot_m = 0
    for g, pm in enumerate(pms):
        with problem(pm) as q:
            q.set_merge_moves(M, P, cqs[g:g + 1])
            q.anneal(Rg, betas[g], 41, replica_offset=2)
            l1, e1, i1 = q.fetch()
            tot_m += q.merges_accepted()
        tot_acc += i1["accepted"]
        assert np.array_equal(lab[g * Rg:(g + 1) * Rg], l1)
        assert np.array_equal(en[g * Rg:(g + 1) * Rg], e1)
    assert info["accepted"] == tot_acc and merges == tot_m and merges > 0


# ---- 3. continuation across merge boundaries = one call --------------------------------------------------------------

@pytest.mark.parametrize("R,cut", [(64, 10), (1100, 7)])
def test_continuation_equals_one_call(R, cut):
    pm = models.build_modularity_potts(graph("s32"), 1.0, 12)
    lo, hi = default_potts_beta_range(pm)
    betas = models.make_beta_schedule(20, (4.0 * lo, hi))
    cq = models.potts_merge_coefficients(pm)
    with problem(pm) as p:
        p.set_merge_moves(5, 24, cq)
        p.anneal(R, betas, 6)
        l1, e1, i1 = p.fetch()
        m1 = p.merges_accepted()
    with problem(pm) as p:
        p.set_merge_moves(5, 24, cq)
        p.anneal(R, betas[:cut], 6)
        _, _, ia = p.fetch()
        ma = p.merges_accepted()
        p.anneal(R, betas[cut:], 6, sweep_offset=cut, continue_run=True)
        l2, e2, ib = p.fetch()
        mb = p.merges_accepted()
    assert np.array_equal(l1, l2) and np.array_equal(e1, e2)
    assert i1["accepted"] == ia["accepted"] + ib["accepted"]
    assert m1 == ma + mb and m1 > 0


def test_call_opening_with_a_merge_phase():
    """A call whose first sweep is a merge point: from random labels (tag-1 words) and from the caller's labels."""
    pm = models.build_modularity_potts(graph("s16"), 1.0, 8)
    lo, hi = default_potts_beta_range(pm)
    betas = models.make_beta_schedule(6, (4.0 * lo, hi))
    cq = models.potts_merge_coefficients(pm)
    R, P = 4, 16
    init = np.random.RandomState(3).randint(0, 8, size=(R, pm.num_variables)).astype(np.uint16)
    for start in (None, init):
        with problem(pm) as p:
            p.set_merge_moves(4, P, cq)
            p.anneal(R, betas, 8, initial_states=start, sweep_offset=4)
            lab, _, info = p.fetch()
            merges = p.merges_accepted()
            rp, cc, vv, dq, dc, cqd, absent, seats = chain_inputs(p, pm)
        dinit = None
        if start is not None:
            dinit = np.zeros((R, len(rp) - 1), dtype=np.uint16)
            dinit[:, seats] = start
        olab, oacc, om = chain2e(rp, cc, vv, dq, dc, cqd, 8, R, betas, 8, 4, P, init=dinit, sweep_offset=4,
                                 absent=absent)
        assert np.array_equal(lab, olab[:, seats]) and info["accepted"] == oacc and merges == om and om > 0


# ---- 4. interval 0 = no merges ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,R", [("mod", 64), ("dqm", 1100)])
def test_interval_zero_is_unchanged(kind, R):
    pm = model_of("s32", kind, 12)
    betas = models.make_beta_schedule(30, default_potts_beta_range(pm))
    cq = models.potts_merge_coefficients(pm)
    out = []
    for setup in (None, 0, 5):
        with problem(pm) as p:
            if setup is not None:
                p.set_merge_moves(setup, 9, cq)
                if setup:
                    p.set_merge_moves(0)
            p.anneal(R, betas, 12)
            lab, en, info = p.fetch()
            out.append((lab, en, info["accepted"], p.kernel_name(), p.launch_count(), p.merges_accepted()))
    for lab, en, acc, name, launches, merges in out[1:]:
        assert np.array_equal(lab, out[0][0]) and np.array_equal(en, out[0][1]) and acc == out[0][2]
        assert name == out[0][3] and "k_potts_merge" not in name and launches == 1 and merges == 0


# ---- 5. errors --------------------------------------------------------------------------------------------------------

def test_merge_abi_errors():
    lib = _lib.load()
    f64p = C.POINTER(C.c_double)
    pm = models.build_modularity_potts(graph("s16"), 1.0, 8)
    cq = np.ascontiguousarray(models.potts_merge_coefficients(pm))
    cqp = cq.ctypes.data_as(f64p)
    with Problem.dense(np.eye(4, dtype=np.float32)) as p:
        assert lib.mi_sa_problem_set_merge_moves(p._h, 5, 8, None) == -1          # not a Potts problem
    with problem(pm) as p:
        assert lib.mi_sa_problem_set_merge_moves(p._h, -1, 8, cqp) == -1          # interval < 0
        assert lib.mi_sa_problem_set_merge_moves(p._h, 5, 0, cqp) == -1           # proposals < 1
        assert lib.mi_sa_problem_set_merge_moves(p._h, 5, 8, None) == -1          # node weights without cq
        assert lib.mi_sa_problem_set_merge_moves(p._h, 0, 8, None) == 0           # off: nothing to check
        assert lib.mi_sa_problem_set_merge_moves(p._h, 5, 8, cqp) == 0
        with pytest.raises(_lib.MiSaError) as e:
            p.set_option("min_cluster_size", 3)
        assert e.value.code == -5
        with pytest.raises(_lib.MiSaError) as e:
            p.tempering_begin([0.5, 1.0], 2, 0, 4)
        assert e.value.code == -5
    dqm = models.build_dqm_potts(graph("s16"), 8, 0.005)
    with problem(dqm) as p:
        p.set_option("min_cluster_size", 3)
        assert lib.mi_sa_problem_set_merge_moves(p._h, 5, 8, None) == -5          # min_cluster_size first
        p.set_option("min_cluster_size", 0)
        assert lib.mi_sa_problem_set_merge_moves(p._h, 5, 8, None) == 0           # unweighted: cq = c_pair
    with problem(dqm) as p:
        p.tempering_begin([0.5, 1.0], 2, 0, 4)
        assert lib.mi_sa_problem_set_merge_moves(p._h, 5, 8, None) == -5          # under tempering


# ---- 6. end to end: the driver with merges ----------------------------------------------------------------------------

def _best_q(ss):
    return float(np.max(ss.info["modularity"]))


def test_clustering_modularity_with_merges_reaches_louvain():
    from scrna_seq_qannealing_clustering_amd import clustering_modularity
    G = bench()
    ss = clustering_modularity(G, 1.0, sampler_kwargs={"seed": 1, "num_sweeps": 4000, "merge_interval": 25})
    assert ss.info["num_sweeps"] == 4000 and ss.info["merges_accepted"] > 0
    assert _best_q(ss) >= LOUVAIN_Q - 0.005
    plain = clustering_modularity(G, 1.0, sampler_kwargs={"seed": 1, "num_sweeps": 4000})
    assert "merges_accepted" not in plain.info
    assert _best_q(plain) < LOUVAIN_Q - 0.005                 # single-site moves alone do not get there in 4000 sweeps
    wide = clustering_modularity(G, 1.0, max_clusters=32, merge_interval=25,
                                 sampler_kwargs={"seed": 1, "num_sweeps": 2000})
    assert _best_q(wide) >= LOUVAIN_Q - 0.01


def test_clustering_modularity_sweep_with_merges():
    from scrna_seq_qannealing_clustering_amd import clustering_modularity, clustering_modularity_sweep
    G = graph("s32")
    kw = {"seed": 3, "num_sweeps": 200, "num_reads": 16}
    sweep = clustering_modularity_sweep(G, [0.6, 1.2], 8, sampler_kwargs=kw, merge_interval=20)
    for gamma, ss in zip((0.6, 1.2), sweep):
        one = clustering_modularity(G, gamma, 8, sampler_kwargs=kw, merge_interval=20)
        assert np.array_equal(ss.record["sample"], one.record["sample"])
        assert np.array_equal(ss.record["energy"], one.record["energy"])
