"""The node-weighted Potts chain (chain 2d) on every kernel form and at the edges of its weights (tests/node_weight_cases.py):
K3f with 8 and 16 label fields, with and without its threshold wavefront; K3 at D = 16, 32 and 64 with 17 to 64 labels and
in its runtime-width form on rows wider than 64; weights that are quantised degrees, zero for a third of the cells, 2^29 on one
cell of a total of exactly 2^30, in {0, 1, 2}, or unrelated to their coefficients.  On every case the device equals
tests/test_modularity_model.py:chain2d bit for bit on the compared replicas (labels; the accepted count where all are
compared) and reports the fp64 energies of the restatement.  tests/test_node_weight_cases.py shows that the cases are sharp."""
import ctypes as C

import networkx as nx
import numpy as np
import pytest

import node_weight_cases as nc
from conftest import load_fixture
from test_gpu_modularity import problem
from test_modularity_model import nx_graph
from scrna_seq_qannealing_clustering_amd import MI355XSampler, _lib, graphs, models

pytestmark = pytest.mark.gpu

RTOL = 1e-9                      # the project's fp64 tolerance (tests/test_gpu_markers.py)


def opened(c, weights=None, model=None):
    """The problem of case ``c`` with its options set."""
    p = problem(c.model if model is None else model, order=c.order, weights=c.weights if weights is None else weights)
    for key, value in c.options:
        p.set_option(key, value)
    return p


def same_inputs(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got.arrays(), want.arrays()))


@pytest.mark.parametrize("name", nc.NAMES)
def test_device_equals_chain2d(name):
    c, ref = nc.case(name), nc.reference(name)
    picks = list(c.picks)
    with opened(c) as p:
        p.anneal(c.R, c.betas, c.seed, replica_offset=c.replica_offset)
        lab, en, info = p.fetch()
        assert p.kernel_name() == c.expected_kernel
        d = nc.device_inputs(p, c)
    assert same_inputs(d, nc.inputs(name))                   # the restatement ran on the seats the device uses
    differ = [r for k, r in enumerate(picks) if not np.array_equal(lab[r], ref.labels[k, d.seats])]
    print("%s: accepted %d (restatement, %d of %d replicas: %d), energies off by %.3g relative"
          % (name, info["accepted"], len(picks), c.R, ref.accepted, np.max(np.abs(en[picks] / ref.energies - 1.0))))
    assert not differ, "replicas %s differ from chain 2d" % differ
    assert np.array_equal(lab[picks], ref.labels[:, d.seats])
    assert info["proposals"] == c.R * len(c.betas) * (len(c.rowptr) - 1)
    if len(picks) == c.R:
        assert info["accepted"] == ref.accepted
    else:
        assert info["accepted"] > ref.accepted
    assert np.allclose(en[picks], ref.energies, rtol=RTOL, atol=0.0)
    # ... which is the host model's fp64 energy of the labels, on every replica
    assert np.allclose(en, c.model.energies(lab), rtol=RTOL, atol=0.0)


@pytest.mark.parametrize("name", nc.CONTINUED)
def test_continued_run_equals_one_run(name):
    c = nc.case(name)
    cut = len(c.betas) // 2 - 1                              # (an odd cut: the pieces differ in length)
    with opened(c) as p:
        p.anneal(c.R, c.betas, c.seed, replica_offset=c.replica_offset)
        l1, e1, i1 = p.fetch()
        assert p.kernel_name() == c.expected_kernel
    with opened(c) as p:
        p.anneal(c.R, c.betas[:cut], c.seed, replica_offset=c.replica_offset)
        _, _, ia = p.fetch()
        p.anneal(c.R, c.betas[cut:], c.seed, replica_offset=c.replica_offset, continue_run=True, sweep_offset=cut)
        l2, e2, ib = p.fetch()
        assert p.kernel_name() == c.expected_kernel
    assert np.array_equal(l1, l2) and np.array_equal(e1, e2)
    assert i1["accepted"] == ia["accepted"] + ib["accepted"] > 0


@pytest.mark.parametrize("name", nc.GROUPED)
def test_groups_equal_single_runs(name):
    """Two resolution groups (mi_sa_problem_set_node_weight_groups): each equals its single-resolution run bit for bit."""
    c = nc.case(name)
    cw2, c64_2, offset2, betas2 = nc.second_group(c)
    assert not np.array_equal(cw2, c.cw)
    with opened(c) as p:
        p.set_node_weight_groups(np.stack([c.cw, cw2]), [c.c64, c64_2], [c.offset, offset2])
        p.anneal(2 * c.R, np.stack([c.betas, betas2]), c.seed, replica_offset=c.replica_offset)
        lab, en, info = p.fetch()
        assert p.kernel_name() == c.expected_kernel
    singles = []
    for g, (cw, c64, offset, betas) in enumerate(((c.cw, c.c64, c.offset, c.betas), (cw2, c64_2, offset2, betas2))):
        pm = c.model
        pm.c_pair = c64
        pm.lin[0] = offset
        with opened(c, weights=(c.wq, cw, c.w64), model=pm) as q:
            q.anneal(c.R, betas, c.seed, replica_offset=c.replica_offset)
            l1, e1, i1 = q.fetch()
            assert q.kernel_name() == c.expected_kernel
        rows = slice(g * c.R, (g + 1) * c.R)
        assert np.array_equal(lab[rows], l1) and np.array_equal(en[rows], e1)
        assert np.allclose(e1, pm.energies(l1), rtol=RTOL, atol=0.0)
        singles.append((l1, i1["accepted"]))
    assert info["accepted"] == singles[0][1] + singles[1][1]
    assert not np.array_equal(singles[0][0], singles[1][0])                # (the groups are different runs)
    # ... and the first group is the run tests/test_node_weight_cases.py holds sharp
    ref = nc.reference(name)
    assert np.array_equal(lab[list(c.picks)], ref.labels[:, nc.inputs(name).seats])


def test_weight_total_at_the_limit():
    """mi_sa_problem_set_node_weights: a total of exactly 2^30 is taken, 2^30 + 1 and a negative weight are MI_EINVAL (-1)
    before anything reaches the device, and the handle anneals afterwards -- on the weights it accepted."""
    lib = _lib.load()
    name = "d16_k8_hub"
    c, ref = nc.case(name), nc.reference(name)
    n = len(c.rowptr) - 1
    assert int(c.wq.astype(np.int64).sum()) == 2 ** 30

    def call(p, q, cw):
        # (the problem's seats: the caller's order -> the device's, holes 0, as Problem.set_node_weights)
        dq = np.zeros(p.n_dev, dtype=np.int32)
        dc = np.zeros(p.n_dev, dtype=np.float32)
        cols = np.arange(n) if p._inv is None else p._inv
        dq[cols] = q
        dc[cols] = cw
        return lib.mi_sa_problem_set_node_weights(p._h, dq.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  dc.ctypes.data_as(C.POINTER(C.c_float)), None)

    over = c.wq.copy()
    over[n - 1] += 1                                         # (the last variable: the total passes the limit at the very end)
    negative = c.wq.copy()
    negative[3] = -1
    unit = (np.ones(n, dtype=np.int32), np.full(n, np.float32(c.c64)), np.ones(n))
    with opened(c, weights=unit) as p:
        assert call(p, c.wq, c.cw) == 0                      # sum wq == 2^30
        assert call(p, over, c.cw) == -1                     # 2^30 + 1
        assert call(p, negative, c.cw) == -1
        # the refused calls left the accepted weights in place: the run of the case
        p.anneal(c.R, c.betas, c.seed, replica_offset=c.replica_offset)
        lab, _, info = p.fetch(energies=False)
        assert p.kernel_name() == c.expected_kernel
    assert np.array_equal(lab[list(c.picks)], ref.labels[:, nc.inputs(name).seats]) and info["accepted"] > 0
    with opened(c, weights=unit) as p:                       # refused first: the handle keeps the weights it was created with
        assert call(p, over, c.cw) == -1 and call(p, negative, c.cw) == -1
        p.anneal(c.R, c.betas, c.seed, replica_offset=c.replica_offset)
        lab1, _, info1 = p.fetch(energies=False)
    with opened(c, weights=unit) as p:
        p.anneal(c.R, c.betas, c.seed, replica_offset=c.replica_offset)
        lab2, _, info2 = p.fetch(energies=False)
    assert np.array_equal(lab1, lab2) and info1["accepted"] == info2["accepted"] > 0


def test_isolated_nodes_end_to_end():
    """A golden graph and three isolated nodes through the sampler: the isolated nodes weigh 0 on the device, and the best
    energy is the networkx modularity of the labels returned with it."""
    fx = load_fixture("noisy_circles")
    iso = ["iso0", "iso1", "iso2"]
    nodes = fx.nodes[:100] + iso[:1] + fx.nodes[100:] + iso[1:]
    index = {v: i for i, v in enumerate(nodes)}
    eu = [index[fx.nodes[a]] for a in fx.eu.tolist()]
    ev = [index[fx.nodes[b]] for b in fx.ev.tolist()]
    G = graphs.graph_from_edges(nodes, eu, ev, fx.w)
    pm = models.build_modularity_potts(G, 1.0, 8)
    assert pm.variables == nodes
    wq, cw, w64 = models.potts_node_weights(pm)
    at = [index[v] for v in iso]
    assert not wq[at].any() and not cw[at].any() and not w64[at].any()
    assert np.all(np.delete(wq, at) > 0)
    ss = MI355XSampler().sample_dqm(pm, num_reads=32, num_sweeps=200, seed=3)
    best = ss.first
    lab = np.array([best.sample[v] for v in nodes])
    assert best.energy == float(np.min(ss.record["energy"]))
    H = nx_graph(G)
    assert list(H.nodes) == nodes and all(H.degree(v) == 0 for v in iso)
    parts = [set(nodes[i] for i in np.flatnonzero(lab == q)) for q in np.unique(lab)]
    ref = nx.community.modularity(H, parts, weight="weight", resolution=1.0)
    assert -best.energy / pm.info["m"] == pytest.approx(ref, rel=1e-9)
    assert ref > 0.3                                         # (an annealed labelling: far from a random one's Q ~ 0)
