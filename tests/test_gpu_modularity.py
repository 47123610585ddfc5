"""Node weights on the Potts kernels (chain 2d, mi_sa_problem_set_node_weights) and the modularity driver on the GPU:
unit weights reproduce the unweighted chain, modularity models reproduce the test-side restatement of chain 2d bit for
bit on K3f and K3, and clustering_modularity reaches networkx Louvain's modularity on the bench graph."""
import ctypes as C

import networkx as nx
import numpy as np
import pytest

from conftest import load_fixture
from test_modularity_model import bench_graph, chain2d, nx_graph
from scrna_seq_qannealing_clustering_amd import MI355XSampler, _lib, models
from scrna_seq_qannealing_clustering_amd.engine import Problem
from scrna_seq_qannealing_clustering_amd.sampler import default_potts_beta_range

pytestmark = pytest.mark.gpu

_BENCH = {}


def bench():
    if "G" not in _BENCH:
        _BENCH["G"] = bench_graph()
    return _BENCH["G"]


def graph(name):
    """``bench``: the bench graph; ``s16`` / ``s32``: small synthetic SNN graphs whose padded layout is free of in-slot
    edges (K3f, 16 / 32 adjacency entries); otherwise a golden graph (too dense to pad: K3 with in-slot edges)."""
    if name == "bench":
        return bench()
    if name in ("s16", "s32"):
        from scrna_seq_qannealing_clustering_amd import graphs
        k, o = (5, 15) if name == "s16" else (8, 30)
        nodes, eu, ev, w, _ = graphs.synthetic_snn(640, k, 15, o, 6, seed=1, spread=3.0)
        return graphs.EdgeListGraph(nodes, eu, ev, w)
    return load_fixture(name).graph()


def f32(a):
    return np.asarray(a, dtype=np.float32)


def problem(pm, order="padded", weights=None):
    """The sampler's problem for ``pm``; ``weights = (wq, cw, w64)`` (default: the model's own, if any)."""
    nw = models.potts_node_weights(pm) if weights is None else (None if weights is False else weights)
    return Problem.potts_csr(pm.rowptr, pm.col, f32(pm.val), float(np.float32(pm.c_pair)), pm.num_variables,
                             pm.num_cases, lin_offset=pm.lin_offset, order=order,
                             energy_model=(pm.val, pm.c_pair), node_weights=nw)


def device_model(p, pm, wq, cw):
    """The model as the device sweeps it (padded / permuted seats): CSR, fp32 values, weights, holes, seat of each variable."""
    seats = np.arange(pm.num_variables) if p._inv is None else np.asarray(p._inv)
    rp, cc, vv = models.pad_csr(pm.rowptr, pm.col, pm.val, seats, p.n_dev)
    dq = np.zeros(p.n_dev, dtype=np.int64)
    dc = np.zeros(p.n_dev, dtype=np.float32)
    dq[seats] = wq
    dc[seats] = cw
    absent = np.ones(p.n_dev, dtype=bool)
    absent[seats] = False
    return rp, cc, f32(vv), dq, dc, absent, seats


# ---- 1. unit weights through set_node_weights equal the unweighted problem ----------------------------------------

@pytest.mark.parametrize("name,K,R,k3", [("bench", 8, 64, 0), ("bench", 16, 1100, 0), ("s32", 8, 1100, 0),
                                         ("s32", 16, 64, 0), ("bench", 16, 64, 2), ("s32", 8, 64, 2)])
def test_unit_weights_equal_unweighted(name, K, R, k3):
    G = graph(name)
    pm = models.build_dqm_potts(G, K, 0.005)
    n = pm.num_variables
    betas = models.make_beta_schedule(24, default_potts_beta_range(pm))
    unit = (np.ones(n, dtype=np.int32), np.full(n, np.float32(pm.c_pair), dtype=np.float32), np.ones(n))
    out = []
    for nw in (None, unit):
        with problem(pm, weights=nw) as p:
            if k3:
                p.set_option("k3_fast", k3)
            p.anneal(R, betas, 21, replica_offset=2)
            lab, en, info = p.fetch()
            out.append((lab, en, info["accepted"], p.kernel_name()))
    (l0, e0, a0, k0), (l1, e1, a1, k1) = out
    D = 16 if name == "bench" else 32
    if k3:
        assert k0 == "k_anneal_potts<%d>" % D and k1 == "k_anneal_potts<%d, weighted>" % D
    else:
        tw = ", tw" if R <= 1024 else ""
        assert k0 == "k_anneal_potts_fast<%d, %d%s>" % (D, 8 if K <= 8 else 16, tw)
        assert k1 == "k_anneal_potts_fast<%d, %d%s, weighted>" % (D, 8 if K <= 8 else 16, tw)
    assert np.array_equal(l0, l1) and a0 == a1 and a0 > 0
    assert np.allclose(e0, e1, rtol=1e-12, atol=0.0)


# ---- 2. modularity models: the device equals the restatement of chain 2d ----------------------------------------------

@pytest.mark.parametrize("name,order,k3,K,kernel", [
    ("s16", "padded", 0, 2, "k_anneal_potts_fast<16, 8, tw, weighted>"),
    ("s16", "padded", 0, 12, "k_anneal_potts_fast<16, 16, tw, weighted>"),
    ("s32", "padded", 0, 8, "k_anneal_potts_fast<32, 8, tw, weighted>"),
    ("s32", "padded", 0, 16, "k_anneal_potts_fast<32, 16, tw, weighted>"),
    ("noisy_circles", "padded", 0, 12, "k_anneal_potts<32, weighted>"),
    ("noisy_moons", "padded", 0, 2, "k_anneal_potts<32, weighted>"),
    ("aniso", "slots", 2, 8, "k_anneal_potts<32, weighted>"),
    ("aniso", "slots", 2, 16, "k_anneal_potts<32, weighted>"),
    ("blobs", "slots", 0, 12, "k_anneal_potts<64, weighted>"),
    ("varied", "padded", 0, 2, "k_anneal_potts<64, weighted>"),
])
def test_modularity_device_equals_restatement(name, order, k3, K, kernel):
    G = graph(name)
    pm = models.build_modularity_potts(G, 0.8, K)
    wq, cw, w64 = models.potts_node_weights(pm)
    betas = models.make_beta_schedule(12, default_potts_beta_range(pm))
    R, pick = 8, [0, 5]
    with problem(pm, order=order) as p:
        if k3:
            p.set_option("k3_fast", k3)
        p.anneal(R, betas, 9, replica_offset=4)
        lab, en, info = p.fetch()
        assert p.kernel_name() == kernel
        rp, cc, vv, dq, dc, absent, seats = device_model(p, pm, wq, cw)
    if not kernel.startswith("k_anneal_potts_fast"):
        assert any(np.any((cc[rp[i]:rp[i + 1]] >> 6) == (i >> 6)) for i in range(len(rp) - 1))   # in-slot edges
    olab, _, _ = chain2d(rp, cc, vv, dq, dc, K, R, betas, 9, replica_offset=4, absent=absent, replicas=pick)
    assert np.array_equal(lab[pick], olab[:, seats])
    assert info["accepted"] > 0
    # energies: the host model in fp64, and -E/m the modularity
    assert np.allclose(en, pm.energies(lab), rtol=1e-9, atol=1e-12)


def test_modularity_full_size_replay():
    """Bench graph, gamma = 1, K = 16, 4096 replicas x 200 sweeps: two replicas' last 20 sweeps replayed."""
    G = bench()
    pm = models.build_modularity_potts(G, 1.0, 16)
    wq, cw, w64 = models.potts_node_weights(pm)
    betas = models.make_beta_schedule(200, default_potts_beta_range(pm))
    R = 4096
    with problem(pm) as p:
        p.anneal(R, betas[:180], 13)
        mid, _, _ = p.fetch(energies=False)
        p.anneal(R, betas[180:], 13, sweep_offset=180, continue_run=True)
        lab, en, info = p.fetch()
        assert p.kernel_name() == "k_anneal_potts_fast<16, 16, weighted>"
        rp, cc, vv, dq, dc, absent, seats = device_model(p, pm, wq, cw)
    pick = [7, 3001]
    init = np.zeros((2, len(rp) - 1), dtype=np.uint16)
    init[:, seats] = mid[pick]
    olab, _, _ = chain2d(rp, cc, vv, dq, dc, 16, R, betas[180:], 13, init=init, sweep_offset=180, absent=absent,
                         replicas=pick)
    assert np.array_equal(lab[pick], olab[:, seats])
    # 5. energies: device fp64 = host model, and -E/m = networkx modularity
    best = int(np.argmin(en))
    sub = np.argsort(en)[:8]
    assert np.allclose(en[sub], pm.energies(lab[sub]), rtol=1e-9, atol=0.0)
    H = nx_graph(G)
    nodes = list(H.nodes)
    parts = [set(nodes[i] for i in np.flatnonzero(lab[best] == q)) for q in np.unique(lab[best])]
    ref = nx.community.modularity(H, parts, weight="weight", resolution=1.0)
    assert -en[best] / pm.info["m"] == pytest.approx(ref, rel=1e-9)


# ---- 4. continuation ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [64, 1100])
def test_continuation_equals_one_run(R):
    pm = models.build_modularity_potts(graph("s32"), 1.0, 12)
    betas = models.make_beta_schedule(40, default_potts_beta_range(pm))
    with problem(pm) as p:
        p.anneal(R, betas, 5)
        l1, e1, i1 = p.fetch()
    with problem(pm) as p:
        p.anneal(R, betas[:20], 5)
        _, _, ia = p.fetch()
        p.anneal(R, betas[20:], 5, sweep_offset=20, continue_run=True)
        l2, e2, ib = p.fetch()
    assert np.array_equal(l1, l2)
    assert np.array_equal(e1, e2)
    assert i1["accepted"] == ia["accepted"] + ib["accepted"]


# ---- 6. end to end --------------------------------------------------------------------------------------------------

def test_clustering_modularity_reaches_louvain():
    from scrna_seq_qannealing_clustering_amd import clustering_modularity
    G = bench()
    ss = clustering_modularity(G, resolution=1.0, sampler_kwargs={"seed": 1})
    Q = np.asarray(ss.info["modularity"])
    assert Q.shape == (len(ss.record),)
    assert np.allclose(Q, -ss.record["energy"] / models.build_modularity_potts(G, 1.0, 16).info["m"], rtol=0, atol=0)
    assert float(Q.max()) >= 0.8229 - 0.005                   # networkx Louvain, seed 0: Q = 0.8229
    assert ss.info["num_reads"] == 256 and ss.info["num_sweeps"] == 16000


# ---- 7. errors ------------------------------------------------------------------------------------------------------

def test_node_weight_errors():
    lib = _lib.load()
    pm = models.build_modularity_potts(load_fixture("blobs").graph(), 1.0, 8)
    wq, cw, w64 = models.potts_node_weights(pm)
    n = pm.num_variables

    def call(p, q, c):
        q = np.ascontiguousarray(q, dtype=np.int32)
        c = np.ascontiguousarray(c, dtype=np.float32)
        return lib.mi_sa_problem_set_node_weights(p._h, q.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  c.ctypes.data_as(C.POINTER(C.c_float)), None)

    with problem(pm, weights=False) as p:
        bad = wq.copy()
        bad[3] = -1
        assert call(p, bad, cw) == -1                          # MI_EINVAL: a negative weight
        assert call(p, np.full(n, 1 << 24), cw) == -1          # MI_EINVAL: sum > 2^30
        assert call(p, wq, cw) == 0
        assert p.set_option("min_cluster_size", 0) is None
        with pytest.raises(_lib.MiSaError) as e:
            p.set_option("min_cluster_size", 3)
        assert e.value.code == -5                              # MI_EUNSUPPORTED
    with problem(pm, weights=False) as p:
        p.set_option("min_cluster_size", 3)
        assert call(p, wq, cw) == -5
    with Problem.dense(np.eye(4, dtype=np.float32)) as p:           # MI_EINVAL: not a Potts problem
        assert call(p, np.ones(4), np.ones(4)) == -1
    with pytest.raises(ValueError):
        MI355XSampler().sample_dqm(pm, num_reads=4, num_sweeps=4, min_cluster_size=2)
