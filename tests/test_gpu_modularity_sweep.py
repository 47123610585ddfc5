"""Resolution groups on the GPU (mi_sa_problem_set_node_weight_groups): group g of a grouped run is the single-resolution
run of its own coefficients, schedule and energy constants with the same seed, bit for bit -- against the device's
single runs and the test-side restatement of chain 2d, on K3f (with and without its threshold wavefront) and K3; G = 1
set explicitly changes nothing; a grouped run continued in two pieces equals one run; the sweep driver equals
clustering_modularity per resolution; and the errors of the C ABI."""
import ctypes as C

import networkx as nx
import numpy as np
import pytest

from test_gpu_modularity import bench, device_model, graph, problem
from test_modularity_model import chain2d, nx_graph
from scrna_seq_qannealing_clustering_amd import _lib, models
from scrna_seq_qannealing_clustering_amd.engine import Problem
from scrna_seq_qannealing_clustering_amd.sampler import default_potts_beta_range

pytestmark = pytest.mark.gpu

GAMMAS = (0.5, 0.8, 1.3)


def sweep_inputs(name, K, sweeps=12):
    pms = models.build_modularity_sweep(graph(name), GAMMAS, K)
    betas = np.stack([models.make_beta_schedule(sweeps, default_potts_beta_range(pm)) for pm in pms])
    return pms, models.potts_node_weight_groups(pms), betas


def grouped_problem(pms, groups, order="padded"):
    wq, cw, w64, c64, offset = groups
    p = problem(pms[0], order=order)
    p.set_node_weight_groups(cw, c64, offset)
    return p


# ---- 1. group g = the single run at gamma_g = chain 2d -------------------------------------------------------------

@pytest.mark.parametrize("name,order,k3,K,Rg,kernel", [
    ("s16", "padded", 0, 8, 6, "k_anneal_potts_fast<16, 8, tw, weighted>"),
    ("s16", "padded", 0, 16, 6, "k_anneal_potts_fast<16, 16, tw, weighted>"),
    ("s32", "padded", 0, 8, 6, "k_anneal_potts_fast<32, 8, tw, weighted>"),
    ("s32", "padded", 0, 16, 6, "k_anneal_potts_fast<32, 16, tw, weighted>"),
    ("s16", "padded", 0, 8, 344, "k_anneal_potts_fast<16, 8, weighted>"),
    ("s16", "padded", 0, 16, 344, "k_anneal_potts_fast<16, 16, weighted>"),
    ("s32", "padded", 0, 8, 344, "k_anneal_potts_fast<32, 8, weighted>"),
    ("s32", "padded", 0, 16, 344, "k_anneal_potts_fast<32, 16, weighted>"),
    ("noisy_circles", "padded", 0, 12, 6, "k_anneal_potts<32, weighted>"),
    ("blobs", "slots", 0, 12, 6, "k_anneal_potts<64, weighted>"),
])
def test_group_equals_single_run_and_restatement(name, order, k3, K, Rg, kernel):
    pms, groups, betas = sweep_inputs(name, K)
    wq, cw, w64, c64, offset = groups
    nG = len(pms)
    seed, ro = 17, 3
    with grouped_problem(pms, groups, order) as p:
        if k3:
            p.set_option("k3_fast", k3)
        p.anneal(nG * Rg, betas, seed, replica_offset=ro)
        lab, en, info = p.fetch()
        assert p.kernel_name() == kernel
        rp, cc, vv, dq, _, absent, seats = device_model(p, pms[0], wq, cw[0])
    if not kernel.startswith("k_anneal_potts_fast"):
        assert any(np.any((cc[rp[i]:rp[i + 1]] >> 6) == (i >> 6)) for i in range(len(rp) - 1))   # in-slot edges
    acc = 0
    for g, pm in enumerate(pms):
        rows = slice(g * Rg, (g + 1) * Rg)
        with problem(pm, order=order) as q:
            if k3:
                q.set_option("k3_fast", k3)
            q.anneal(Rg, betas[g], seed, replica_offset=ro)
            l1, e1, i1 = q.fetch()
        assert np.array_equal(lab[rows], l1)
        assert np.allclose(en[rows], e1, rtol=1e-9, atol=1e-12)
        assert np.allclose(en[rows], pm.energies(lab[rows]), rtol=1e-9, atol=1e-12)
        acc += i1["accepted"]
        # the restatement on one replica of the group (its stream: the index inside the group)
        pick = [g % Rg]
        dc = np.zeros(p.n_dev, dtype=np.float32)
        dc[seats] = cw[g]
        olab, _, _ = chain2d(rp, cc, vv, dq, dc, K, Rg, betas[g], seed, replica_offset=ro, absent=absent,
                             replicas=pick)
        assert np.array_equal(lab[g * Rg + pick[0]][None, :], olab[:, seats])
    assert info["accepted"] == acc and acc > 0


# ---- 2. the sweep driver = clustering_modularity per resolution --------------------------------------------------------

def test_sweep_driver_equals_single_resolution_runs():
    from scrna_seq_qannealing_clustering_amd import clustering_modularity, clustering_modularity_sweep
    G = bench()
    res = [0.5, 0.9]
    sweep = clustering_modularity_sweep(G, res, sampler_kwargs={"seed": 1})
    assert len(sweep) == 2
    H = nx_graph(G)
    for gamma, ss in zip(res, sweep):
        one = clustering_modularity(G, gamma, sampler_kwargs={"seed": 1})
        assert ss.info["resolution"] == gamma
        assert np.array_equal(ss.record["sample"], one.record["sample"])
        assert np.array_equal(ss.record["energy"], one.record["energy"])
        assert np.array_equal(ss.record["num_occurrences"], one.record["num_occurrences"])
        assert np.array_equal(ss.info["modularity"], one.info["modularity"])
        assert ss.info["beta_range"] == one.info["beta_range"] and ss.info["num_sweeps"] == 16000
        assert ss.info["batch"]["groups"] == 2 and ss.info["num_reads"] == 256
        comms = nx.community.louvain_communities(H, weight="weight", resolution=gamma, seed=0)
        louvain = nx.community.modularity(H, comms, weight="weight", resolution=gamma)
        assert float(np.max(ss.info["modularity"])) >= louvain - 0.005, (gamma, louvain)


# ---- 3. G = 1 set explicitly = no groups ------------------------------------------------------------------------------

@pytest.mark.parametrize("name,k3,R", [("s16", 0, 40), ("s32", 0, 1100), ("bench", 2, 40)])
def test_one_explicit_group_equals_no_groups(name, k3, R):
    pm = models.build_modularity_potts(graph(name), 0.8, 12)
    wq, cw, w64 = models.potts_node_weights(pm)
    betas = models.make_beta_schedule(20, default_potts_beta_range(pm))
    out = []
    for grouped in (False, True):
        with problem(pm) as p:
            if grouped:
                p.set_node_weight_groups(cw[None, :], [pm.c_pair], [pm.lin_offset])
            if k3:
                p.set_option("k3_fast", k3)
            p.anneal(R, betas, 4, replica_offset=1)
            out.append(p.fetch() + (p.kernel_name(),))
    (l0, e0, i0, k0), (l1, e1, i1, k1) = out
    assert k0 == k1
    assert np.array_equal(l0, l1) and np.array_equal(e0, e1) and i0["accepted"] == i1["accepted"] > 0


# ---- 4. continuation ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Rg", [8, 400])
def test_grouped_continuation_equals_one_run(Rg):
    pms, groups, betas = sweep_inputs("s32", 12, sweeps=40)
    R = len(pms) * Rg
    with grouped_problem(pms, groups) as p:
        p.anneal(R, betas, 5)
        l1, e1, i1 = p.fetch()
    with grouped_problem(pms, groups) as p:
        p.anneal(R, betas[:, :20], 5)
        _, _, ia = p.fetch()
        p.anneal(R, betas[:, 20:], 5, sweep_offset=20, continue_run=True)
        l2, e2, ib = p.fetch()
    assert np.array_equal(l1, l2)
    assert np.array_equal(e1, e2)
    assert i1["accepted"] == ia["accepted"] + ib["accepted"]
    # one shared schedule (no per-group flag) = every group on that schedule
    with grouped_problem(pms, groups) as p:
        p.anneal(R, betas[1], 5)
        l3, _, _ = p.fetch()
    with grouped_problem(pms, groups) as p:
        p.anneal(R, np.stack([betas[1]] * len(pms)), 5)
        l4, _, _ = p.fetch()
    assert np.array_equal(l3, l4)


# ---- 5. errors ------------------------------------------------------------------------------------------------------

def test_node_weight_group_errors():
    lib = _lib.load()
    pms, groups, betas = sweep_inputs("s16", 8)
    wq, cw, w64, c64, offset = groups
    n = pms[0].num_variables

    def call(p, G, c, k=c64, o=offset):
        # (every call below fails before the tables are read)
        c = None if c is None else np.ascontiguousarray(c, dtype=np.float32)
        return lib.mi_sa_problem_set_node_weight_groups(
            p._h, int(G), None if c is None else c.ctypes.data_as(C.POINTER(C.c_float)),
            None if k is None else np.ascontiguousarray(k).ctypes.data_as(C.POINTER(C.c_double)),
            None if o is None else np.ascontiguousarray(o).ctypes.data_as(C.POINTER(C.c_double)))

    big = np.zeros((257, n), dtype=np.float32)
    with problem(pms[0]) as p:
        assert call(p, 3, None) == -1                                     # MI_EINVAL: NULL arguments
        assert call(p, 3, cw, k=None) == -1
        assert call(p, 3, cw, o=None) == -1
        assert call(p, 0, cw) == -1                                       # G < 1
        assert call(p, 257, big, k=np.zeros(257), o=np.zeros(257)) == -1  # G > 256
        p.set_node_weight_groups(cw, c64, offset)                          # (the caller's order -> the padded seats)
        with pytest.raises(_lib.MiSaError) as e:                          # R not a multiple of G
            p.anneal(10, betas, 1)
        assert e.value.code == -1
        with pytest.raises(_lib.MiSaError) as e:                          # per-replica betas
            p.anneal(12, np.ones(12), 1, num_sweeps=4)
        assert e.value.code == -5
        with pytest.raises(_lib.MiSaError) as e:                          # resident temperatures
            p.anneal(12, None, 1, num_sweeps=4)
        assert e.value.code == -5
        with pytest.raises(_lib.MiSaError) as e:                          # tempering
            p.tempering_begin([0.5, 1.0, 2.0], 4, 0, 12)
        assert e.value.code == -5
        probs = (C.c_void_p * 1)(p._h.value)
        assert lib.mi_multi_gpu_anneal(probs, 1, 12, 0, 4, betas[0].ctypes.data_as(C.POINTER(C.c_double)), 1, 0) == -5
        p.anneal(12, betas, 1)
        lab, en, _ = p.fetch()
        with pytest.raises(_lib.MiSaError) as e:                          # best across different objectives
            p.best()
        assert e.value.code == -5
        assert call(p, 3, cw) == -1                                       # after the first anneal
    with problem(pms[0], weights=False) as p:
        assert call(p, 3, cw) == -1                                       # no node weights
    with pytest.raises(ValueError):
        with grouped_problem(pms, groups) as p:
            p.anneal(12, betas[:2], 1)                                    # betas for 2 of the 3 groups
