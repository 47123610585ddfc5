"""The host side of ``split_disconnected`` and of the batched components entry (no GPU): the energy evaluator for
labellings with more labels than ``num_cases`` against the model's own and against hand-counted pair terms, the
renumbering helper, the argument validation of ``mi_graph_components`` (it happens before any device work) and the
keyword combinations the samplers refuse before any GPU work."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_fixture
from scrna_seq_qannealing_clustering_amd import _lib, clustering, metrics, models
from scrna_seq_qannealing_clustering_amd import sampler as smod

EINVAL, EUNSUPPORTED = -1, -5
RTOL = 1e-9                                   # the project's fp64 energy tolerance


def fixture_models(name, K=4):
    G = load_fixture(name).graph()
    return [models.build_dqm_potts(G, K, 0.005), models.build_modularity_potts(G, 1.0, K),
            models.build_modularity_potts(G, 2.5, K)]


def term_scale(pm):
    """Sum of the absolute values of everything an energy of ``pm`` can add up: the couplings, the pair term over all
    pairs and the offset.  Two fp64 evaluations that add the same terms in different orders differ by a few ulp of THIS
    (the all-in-one-cluster modularity energy is 0 up to that cancellation), so for labellings that cancel like that the
    project's 1e-9 is taken relative to it; every other comparison here is relative to the energy itself."""
    w = np.ones(pm.num_variables) if pm.node_weight is None else np.asarray(pm.node_weight, dtype=np.float64)
    return 0.5 * float(np.sum(np.abs(pm.val))) + abs(pm.c_pair) * 0.5 * float(np.sum(w)) ** 2 + abs(pm.lin_offset)


# ---- 1. the host energy evaluator ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["blobs", "noisy_circles", "varied"])
def test_energies_any_equals_the_model_energy_within_num_cases(name):
    rng = np.random.default_rng(len(name))
    for pm in fixture_models(name):
        L = rng.integers(0, pm.num_cases, (6, pm.num_variables))
        L[5] = 0                                                    # one cluster
        want = pm.energies(L)
        got = models.potts_energies_any(pm, L)
        assert got.shape == (6,) and got.dtype == np.float64
        assert np.all(np.abs(got - want)[:5] <= RTOL * np.maximum(np.abs(got), np.abs(want))[:5])
        assert abs(got[5] - want[5]) <= RTOL * term_scale(pm)       # (the one-cluster row cancels to ~0: see term_scale)
        assert models.potts_energies_any(pm, L[2])[0] == got[2]     # a 1-D labelling is one row
        # the labels' names do not matter: any integers, more distinct values than num_cases allowed
        assert np.array_equal(models.potts_energies_any(pm, L * 1000 - 3), got)
    with pytest.raises(ValueError):
        models.potts_energies_any(pm, np.zeros((2, 5)))


def removed_pair_terms(pm, before, after):
    """sum of the pair terms of the pairs that share a label in ``before`` and not in ``after``, counted pair by pair"""
    n = pm.num_variables
    w = np.ones(n) if pm.node_weight is None else np.asarray(pm.node_weight, dtype=np.float64)
    iu, ju = np.triu_indices(n, 1)
    gone = (before[iu] == before[ju]) & (after[iu] != after[ju])
    return float(np.sum(pm.c_pair * w[iu[gone]] * w[ju[gone]])), iu[gone], ju[gone]


@pytest.mark.parametrize("name,sizes", [("blobs", [86, 85, 85]), ("noisy_circles", [128, 128])])
def test_refined_energy_is_lower_by_exactly_the_removed_pair_terms(name, sizes):
    f = load_fixture(name)
    n = len(f.nodes)
    comp = f.components()
    comp = np.unique(comp, return_inverse=True)[1].reshape(-1)
    assert sorted(np.bincount(comp).tolist(), reverse=True) == sizes
    rng = np.random.default_rng(n)
    # disconnected labellings made by hand: every component under one label; the first two components merged; a random
    # 2-colouring inside the components on top of a merge
    hand = [np.zeros(n, dtype=np.int64), comp // 2, rng.integers(0, 2, n) + 2 * (comp // 2)]
    for pm in fixture_models(name, K=4):
        edges = set(zip(*[a.tolist() for a in smod.model_edges(pm)]))
        for before in hand:
            after = before * len(sizes) + comp                      # the split along the components
            e0, e1 = models.potts_energies_any(pm, before)[0], models.potts_energies_any(pm, after)[0]
            removed, iu, ju = removed_pair_terms(pm, before, after)
            assert removed > 0.0 and not (set(zip(iu.tolist(), ju.tolist())) & edges)   # no coupling is cut
            assert e1 < e0
            assert abs((e0 - e1) - removed) <= RTOL * max(abs(e0), abs(e1), removed)
            assert abs(e0 - pm.energies(before[None, :])[0]) <= RTOL * term_scale(pm)
            # a labelling whose clusters are connected already keeps its energy
            assert models.potts_energies_any(pm, comp)[0] == models.potts_energies_any(pm, comp * 7 + 1)[0]


def test_renumber_by_first_cell():
    A = np.array([[5, 5, 2, 9, 2, 0], [0, 1, 2, 3, 4, 5], [3, 3, 3, 3, 3, 3], [9, 0, 9, 0, 4, 4]])
    want = np.array([[0, 0, 1, 2, 1, 3], [0, 1, 2, 3, 4, 5], [0, 0, 0, 0, 0, 0], [0, 1, 0, 1, 2, 2]])
    out = metrics.renumber_by_first_cell(A)
    assert out.dtype == np.int32 and np.array_equal(out, want)
    assert np.array_equal(metrics.renumber_by_first_cell(A[3:]), want[3:])


# ---- 2. argument validation of mi_graph_components (before any device work) -----------------------------------------

def call(rowptr, col, n, B=1, flags=0, out=True, cnt=True, L=None, keep=None):
    i32p = C.POINTER(C.c_int32)
    rp = None if rowptr is None else np.ascontiguousarray(rowptr, dtype=np.int32)
    cc = None if col is None else np.ascontiguousarray(col, dtype=np.int32)
    o = np.zeros((max(B, 1), max(n, 1)), dtype=np.int32) if out else None
    c = np.zeros(max(B, 1), dtype=np.int32) if cnt else None
    ptr = (lambda a, t: None if a is None else a.ctypes.data_as(t))
    return _lib.load().mi_graph_components(ptr(rp, i32p), ptr(cc, i32p), n, ptr(L, C.POINTER(C.c_uint16)),
                                           ptr(keep, C.POINTER(C.c_uint8)), B, 0, flags, ptr(o, i32p), ptr(c, i32p), None)


def test_graph_components_argument_validation():
    lib = _lib.load()
    good_rp, good_col = [0, 1, 2, 2], [1, 0]
    cases = [
        (dict(rowptr=None, col=good_col, n=3), b"NULL"),
        (dict(rowptr=good_rp, col=good_col, n=3, out=False), b"NULL"),
        (dict(rowptr=good_rp, col=good_col, n=3, cnt=False), b"NULL"),
        (dict(rowptr=[0], col=[], n=0), b"n must be"),
        (dict(rowptr=good_rp, col=good_col, n=-3), b"n must be"),
        (dict(rowptr=good_rp, col=good_col, n=3, B=0), b"B must be"),
        (dict(rowptr=good_rp, col=good_col, n=3, B=-2), b"B must be"),
        (dict(rowptr=good_rp, col=good_col, n=3, flags=2), b"flags"),
        (dict(rowptr=[1, 1, 2, 2], col=good_col, n=3), b"rowptr[0]"),
        (dict(rowptr=[0, 2, 1, 2], col=good_col, n=3), b"monotone"),
        (dict(rowptr=good_rp, col=[1, 3], n=3), b"outside"),
        (dict(rowptr=good_rp, col=[-1, 0], n=3), b"outside"),
        (dict(rowptr=good_rp, col=None, n=3), b"col is NULL"),
    ]
    for kw, text in cases:
        assert call(**kw) == EINVAL, kw
        assert text in lib.mi_last_error(), (kw, lib.mi_last_error())
    # B * n beyond the output cap: refused, nothing allocated
    big = np.zeros(1 << 20 | 1, dtype=np.int32)
    o, c = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    i32p = C.POINTER(C.c_int32)
    rc = lib.mi_graph_components(big.ctypes.data_as(i32p), None, 1 << 20, None, None, 1 << 13, 0, 0, o.ctypes.data_as(i32p),
                                 c.ctypes.data_as(i32p), None)
    assert rc == EUNSUPPORTED and b"exceed" in lib.mi_last_error()


def test_python_entry_validates_before_the_library():
    eu, ev = np.array([0, 1]), np.array([1, 2])
    with pytest.raises(ValueError):
        metrics.connected_components((eu, ev), 0)
    with pytest.raises(ValueError):
        metrics.connected_components((eu, np.array([1, 3])), 3)                      # an edge index outside [0, n)
    with pytest.raises(ValueError):
        metrics.connected_components((eu, ev), 3, labels=np.zeros((2, 4)))           # labels of another n
    with pytest.raises(ValueError):
        metrics.connected_components((eu, ev), 3, keep=np.ones((2, 3)))              # keep of another edge count
    with pytest.raises(ValueError):
        metrics.connected_components((eu, ev), 3, labels=np.zeros((2, 3), dtype=int), keep=np.ones((3, 2)))
    rp, col, order = metrics._graph_csr((np.array([2, 0, 2, 1]), np.array([0, 1, 1, 1])), 3)
    assert rp.tolist() == [0, 1, 2, 4] and col.tolist() == [1, 1, 0, 1] and order.tolist() == [1, 3, 0, 2]
    rp2, col2, none = metrics._graph_csr((rp, col), 3)                               # a CSR passes through
    assert none is None and rp2.tolist() == rp.tolist() and col2.tolist() == col.tolist()
    L = metrics._labels_u16(np.array([[70000, -1, 70000], [1, 2, 1]]), 3)
    assert L.dtype == np.uint16 and L.tolist() == [[1, 0, 1], [0, 1, 0]]
    assert metrics._labels_u16(np.array([65535, 0, 7]), 3).tolist() == [[65535, 0, 7]]


# ---- 3. the refused keyword combinations -------------------------------------------------------------------------------------

class NoGpuSampler(smod.MI355XSampler):
    """the sampler without its library check; a test that reaches the GPU fails on the missing device"""

    def __init__(self):
        self.device, self.replica_offset = 0, 0


def test_split_disconnected_refusals_come_before_any_gpu_work():
    assert "split_disconnected" in smod.MI355XSampler.parameters
    G = load_fixture("blobs").graph()
    pm = models.build_modularity_potts(G, 1.0, 4)
    smod._check_split({}, 5, [pm])                                  # off: nothing to check
    smod._check_split({"split_disconnected": True}, 0, [pm])
    with pytest.raises(ValueError, match="min_cluster_size"):
        smod._check_split({"split_disconnected": True}, 5, [pm])
    neg = models.PottsModel(pm.variables, pm.num_cases, pm.rowptr, pm.col, pm.val, -0.25, pm.lin)
    with pytest.raises(ValueError, match="non-negative pair coefficient"):
        smod._check_split({"split_disconnected": True}, 0, [pm, neg])
    s = NoGpuSampler()
    cq = models.build_cqm_potts(G, 4, 20)
    with pytest.raises(ValueError, match="min_cluster_size"):
        s.sample_dqm(cq, split_disconnected=True, num_reads=4, num_sweeps=1)
    with pytest.raises(ValueError, match="min_cluster_size"):
        s.sample_dqm(models.build_dqm_potts(G, 4, 0.005), split_disconnected=True, min_cluster_size=3, num_reads=4, num_sweeps=1)
    with pytest.raises(ValueError, match="non-negative pair coefficient"):
        s.sample_dqm(neg, split_disconnected=True, num_reads=4, num_sweeps=1)
    with pytest.raises(ValueError, match="min_cluster_size"):
        s.sample_dqm_many(models.build_modularity_sweep(G, [0.5, 1.0], 4), split_disconnected=True, min_cluster_size=3)
    with pytest.raises(ValueError, match="Potts samplers"):
        s.sample_qubo({(0, 0): -1.0, (0, 1): 2.0}, split_disconnected=True)
    with pytest.raises(ValueError, match="min_cluster_size"):
        clustering.clustering_cqm(G, 4, 20, sampler=s, sampler_kwargs=dict(split_disconnected=True))
    for fn in (clustering.clustering_dqm, clustering.clustering_modularity, clustering.clustering_modularity_sweep):
        assert "split_disconnected" in fn.__code__.co_varnames
