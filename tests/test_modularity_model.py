"""Modularity as a Potts model with node weights (models.build_modularity_potts, chain 2d): the model against
networkx, the quantisation of the degrees, and a test-side restatement of chain 2d that must
reproduce chain 2c (oracle/sa_oracle.c) with unit weights."""
import ctypes
import ctypes.util

import networkx as nx
import numpy as np
import pytest

from conftest import GRAPH_NAMES, load_fixture
from oracle import sa_oracle as so
from scrna_seq_qannealing_clustering_amd import metrics, models

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_float]


def fmaf(a, b, c):
    """fp32 fused multiply-add, rounded once (libm)."""
    return np.float32(_libm.fmaf(float(a), float(b), float(c)))


def chain2d(rowptr, col, val, wq, cw, K, R, betas, seed, replica_offset=0, init=None, sweep_offset=0,
            absent=None, replicas=None, energy=None, trace=None):
    """Chain 2d, sequentially: the Potts chain 2c with the uniform size term replaced by integer node weights,
        dE = fmaf(cw_i, (float)(W_b - W_a + wq_i), hd),  accepted iff dE < neglog_u(word0) * T.
    ``replicas``: the replica ids to run (default 0..R-1, plus ``replica_offset``); ``init`` rows follow them.
    ``energy = (val64, w64, c64, offset)``: also the fp64 energies as the device reports them.
    ``trace``: a list that receives (row of ``replicas``, sweep, i, W_b - W_a + wq_i, accepted) per evaluated move.
    Returns (labels, accepted, energies or None)."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    val = np.asarray(val, dtype=np.float32)
    wq = np.asarray(wq, dtype=np.int64)
    cw = np.asarray(cw, dtype=np.float32)
    n = len(rowptr) - 1
    hole = np.zeros(n, dtype=bool) if absent is None else np.asarray(absent, dtype=bool)
    temps = [np.float32(1.0 / b) for b in np.asarray(betas, dtype=np.float64)]
    ids = list(range(R)) if replicas is None else list(replicas)
    out = np.zeros((len(ids), n), dtype=np.uint16)
    acc = 0
    rows = [(col[rowptr[i]:rowptr[i + 1]].tolist(), val[rowptr[i]:rowptr[i + 1]].tolist()) for i in range(n)]
    for k, r in enumerate(ids):
        gid = replica_offset + r
        if init is not None:
            lab = [int(x) for x in init[k]]
        else:
            lab = [so.chain_word(seed, i, 0, gid, 1) % K for i in range(n)]
        W = [0] * K
        for i in range(n):
            if hole[i]:
                lab[i] = 0
            else:
                W[lab[i]] += int(wq[i])
        for s, T in enumerate(temps):
            for i in range(n):
                if hole[i]:
                    continue
                a = lab[i]
                b = (a + 1 + so.chain_word(seed, i, s + sweep_offset, gid, 2) % (K - 1)) % K
                hd = np.float32(0.0)
                cs, vs = rows[i]
                for j, v in zip(cs, vs):
                    lj = lab[j]
                    if lj == b:
                        hd = np.float32(hd + np.float32(v))
                    elif lj == a:
                        hd = np.float32(hd - np.float32(v))
                d = W[b] - W[a] + int(wq[i])
                dE = fmaf(cw[i], np.float32(d), hd)
                thr = np.float32(so.neglog_u(so.chain_word(seed, i, s + sweep_offset, gid, 0))) * T
                if trace is not None:
                    trace.append((k, s, i, d, bool(dE < thr)))
                if dE < thr:
                    lab[i] = b
                    W[a] -= int(wq[i])
                    W[b] += int(wq[i])
                    acc += 1
        out[k] = lab
    en = None
    if energy is not None:
        val64, w64, c64, offset = energy
        en = device_energies(rowptr, col, val64, w64, c64, offset, out, hole, K)
    return out, acc, en


def device_energies(rowptr, col, val64, w64, c64, offset, L, hole, K):
    """sum_{edges, same label} val64 + c64 / 2 sum_q (W64_q^2 - sum_{i in q} w64_i^2) + offset, per row of L."""
    n = len(rowptr) - 1
    rws = np.repeat(np.arange(n), np.diff(rowptr))
    w64 = np.where(hole, 0.0, np.asarray(w64, dtype=np.float64))
    L = np.asarray(L, dtype=np.int64)
    e = np.empty(L.shape[0])
    up = col > rws
    for r in range(L.shape[0]):
        same = (L[r, rws] == L[r, col]) & up
        W = np.bincount(L[r], weights=w64, minlength=K)
        e[r] = float(np.sum(np.asarray(val64)[same])) + c64 * 0.5 * (float(np.sum(W * W)) - float(np.sum(w64 * w64))) + offset
    return e


def bench_graph():
    import bench
    return bench.build_workload()[4]


def nx_graph(G):
    """A networkx graph with the same nodes (in order) and weighted edges."""
    nodes, eu, ev, w = models.graph_arrays(G)
    H = nx.Graph()
    H.add_nodes_from(nodes)
    H.add_weighted_edges_from((nodes[a], nodes[b], float(c)) for a, b, c in zip(eu, ev, w))
    return H


def _check_model(G, H, resolutions, rng):
    nodes = list(H.nodes)
    for gamma in resolutions:
        pm = models.build_modularity_potts(G, gamma, 16)
        m = pm.info["m"]
        labs = [rng.randint(0, k, size=len(nodes)) for k in (2, 5, 16)]
        comms = nx.community.louvain_communities(H, weight="weight", resolution=gamma, seed=0)
        lv = np.zeros(len(nodes), dtype=np.int64)
        index = {v: i for i, v in enumerate(nodes)}
        for c, members in enumerate(comms):
            for v in members:
                lv[index[v]] = c
        if lv.max() < 16:
            labs.append(lv)
        for L in labs:
            parts = [set(nodes[i] for i in np.flatnonzero(L == q)) for q in np.unique(L)]
            ref = nx.community.modularity(H, parts, weight="weight", resolution=gamma)
            q_model = -pm.energies(L[None, :])[0] / m
            q_host = metrics.modularity(H, L, resolution=gamma)
            # (a random labelling scores Q ~ 0 as a difference of two terms of order 1: 1e-12 relative to those)
            assert q_model == pytest.approx(ref, rel=1e-12, abs=1e-12)
            assert q_host == pytest.approx(ref, rel=1e-12, abs=1e-12)


@pytest.mark.parametrize("name", GRAPH_NAMES)
def test_model_equals_networkx_on_golden_graphs(name):
    G = load_fixture(name).graph()
    _check_model(G, nx_graph(G), (0.5, 0.8, 1.0), np.random.RandomState(1))


def test_model_equals_networkx_on_bench_graph():
    G = bench_graph()
    _check_model(G, nx_graph(G), (0.5, 0.8, 1.0), np.random.RandomState(2))


def test_self_loop_counts_as_networkx():
    H = nx.Graph()
    H.add_weighted_edges_from([(0, 1, 1.0), (1, 2, 2.0), (2, 0, 0.5), (2, 3, 1.5), (3, 4, 1.0), (4, 5, 2.0),
                               (5, 3, 1.0), (4, 4, 0.75)])
    _check_model(H, H, (0.5, 0.8, 1.0), np.random.RandomState(3))


def test_degree_quantisation():
    G = bench_graph()
    pm = models.build_modularity_potts(G, 0.8, 16)
    wq, cw, w64 = models.potts_node_weights(pm)
    e = pm.info["scale_exp"]
    k = np.asarray(pm.node_weight)
    assert int(np.sum(wq.astype(np.int64))) <= 2 ** 30
    assert int(np.sum(np.rint(np.ldexp(k, e + 1)))) > 2 ** 30            # e is the largest such exponent
    assert np.all(np.abs(np.ldexp(wq.astype(np.float64), -e) - k) <= 2.0 ** -(e + 1))
    c = 0.8 / (2.0 * pm.info["m"])
    assert pm.c_pair == c
    assert np.array_equal(cw, (np.ldexp(c, -2 * e) * wq.astype(np.float64)).astype(np.float32))
    assert np.array_equal(w64, k)
    assert pm.info["kind"] == "modularity" and pm.info["resolution"] == 0.8


def test_builder_errors():
    H = nx.Graph()
    H.add_weighted_edges_from([(0, 1, 1.0), (1, 2, -0.5)])
    with pytest.raises(ValueError):
        models.build_modularity_potts(H)
    E = nx.Graph()
    E.add_nodes_from(range(5))
    with pytest.raises(ValueError):
        models.build_modularity_potts(E)
    G = load_fixture("blobs").graph()
    with pytest.raises(ValueError):
        models.build_modularity_potts(G, 1.0, 1)


def test_modularity_beta_range():
    G = bench_graph()
    pm = models.build_modularity_potts(G, 1.0, 16)
    hot, cold = models.modularity_beta_range(pm)
    assert hot == pytest.approx(np.log(100.0) / np.median(pm.node_weight), rel=1e-12)
    rows = np.repeat(np.arange(pm.num_variables), np.diff(pm.rowptr))
    full = np.abs(pm.val + pm.c_pair * pm.node_weight[rows] * pm.node_weight[pm.col])
    assert cold == pytest.approx(np.log(10.0) / full[full > 0].min(), rel=1e-12)
    assert 0.0 < hot < cold


def test_weighted_beta_range():
    from scrna_seq_qannealing_clustering_amd.sampler import default_potts_beta_range
    G = load_fixture("noisy_circles").graph()
    pm = models.build_dqm_potts(G, 8, 0.005)
    assert pm.node_weight is None
    pw = models.PottsModel(pm.variables, pm.num_cases, pm.rowptr, pm.col, pm.val, pm.c_pair, pm.lin,
                           node_weight=np.ones(pm.num_variables))
    # unit weights: the same largest single-move |dE| (the hot end)
    assert default_potts_beta_range(pw)[0] == pytest.approx(default_potts_beta_range(pm)[0], rel=1e-12)
    mod = models.build_modularity_potts(G, 1.0, 8)
    lo, hi = default_potts_beta_range(mod)
    assert 0.0 < lo < hi


def test_restatement_with_unit_weights_is_chain_2c():
    """Chain 2d with wq = 1, cw = c_pair equals the oracle's chain 2c bit for bit (padded layout: holes)."""
    G = load_fixture("noisy_circles").graph()
    K = 8
    pm = models.build_dqm_potts(G, K, 0.005)
    seats = np.arange(256) + (np.arange(256) // 48) * 16             # 48 variables per slot, 16 holes
    n_dev = int(seats[-1]) + 1
    rp, cc, vv = models.pad_csr(pm.rowptr, pm.col, pm.val, seats, n_dev)
    absent = np.ones(n_dev, dtype=np.uint8)
    absent[seats] = 0
    assert absent.sum() > 0
    v32 = vv.astype(np.float32)
    c32 = float(np.float32(pm.c_pair))
    betas = models.make_beta_schedule(12, (0.05, 3.0))
    R = 3
    olab, oen, ostats = so.potts_csr_philox(rp, cc, v32, c32, n_dev, K, R, betas, 91, lin_offset=pm.lin_offset,
                                            replica_offset=5, absent=absent)
    wq = np.where(absent, 0, 1)
    cw = np.full(n_dev, c32, dtype=np.float32)
    lab, acc, en = chain2d(rp, cc, v32, wq, cw, K, R, betas, 91, replica_offset=5, absent=absent,
                           energy=(v32.astype(np.float64), wq.astype(np.float64), c32, pm.lin_offset))
    assert np.array_equal(lab, olab)
    assert acc == int(ostats[1]) and acc > 0
    assert np.allclose(en, oen, rtol=1e-12, atol=1e-12)
