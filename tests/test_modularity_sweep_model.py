"""Resolution sweeps on the host side: models.build_modularity_sweep against build_modularity_potts, the per-group tables
of models.potts_node_weight_groups, the validation of the sweep driver and of the group tables, and the new C-ABI entry
rejecting a NULL handle (no compute: CPU box)."""
import ctypes

import numpy as np
import pytest

from conftest import GRAPH_NAMES, load_fixture
from test_modularity_model import bench_graph
from scrna_seq_qannealing_clustering_amd import _lib, models

RESOLUTIONS = (0.2, 0.5, 0.8, 1.0, 1.6)


def _same_model(a, b):
    assert a.variables == b.variables and a.num_cases == b.num_cases
    for f in ("rowptr", "col", "val", "lin", "node_weight"):
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and np.array_equal(x, y), f
    assert a.c_pair == b.c_pair and a.lin_offset == b.lin_offset
    assert a.info == b.info


def _check_sweep(G, K):
    sweep = models.build_modularity_sweep(G, RESOLUTIONS, K)
    assert len(sweep) == len(RESOLUTIONS)
    singles = [models.build_modularity_potts(G, g, K) for g in RESOLUTIONS]
    for m, s in zip(sweep, singles):
        _same_model(m, s)
    wq, cw, w64, c64, offset = models.potts_node_weight_groups(sweep)
    assert cw.shape == (len(RESOLUTIONS), sweep[0].num_variables) and cw.dtype == np.float32
    for g, s in enumerate(singles):
        swq, scw, sw64 = models.potts_node_weights(s)
        assert np.array_equal(wq, swq) and np.array_equal(w64, sw64)
        assert cw[g].tobytes() == scw.tobytes()                  # bit for bit
        assert c64[g] == s.c_pair and offset[g] == s.lin_offset


@pytest.mark.parametrize("name", GRAPH_NAMES)
def test_sweep_equals_single_models_on_golden_graphs(name):
    _check_sweep(load_fixture(name).graph(), 12)


def test_sweep_equals_single_models_on_bench_graph():
    _check_sweep(bench_graph(), 16)


def test_node_weight_groups_reject_mismatched_models():
    G = load_fixture("blobs").graph()
    a, b = models.build_modularity_sweep(G, (0.5, 1.0), 8)
    with pytest.raises(ValueError):
        models.potts_node_weight_groups([])
    with pytest.raises(ValueError):                                       # another graph
        models.potts_node_weight_groups([a, models.build_modularity_potts(load_fixture("aniso").graph(), 1.0, 8)])
    with pytest.raises(ValueError):                                       # another label count
        models.potts_node_weight_groups([a, models.build_modularity_potts(G, 1.0, 12)])
    with pytest.raises(ValueError):                                       # no node weights
        models.potts_node_weight_groups([a, models.build_dqm_potts(G, 8, 0.5)])
    for f in ("val", "node_weight"):                                      # the same structure, other values
        c = models.PottsModel(b.variables, b.num_cases, b.rowptr, b.col, b.val.copy(), b.c_pair, b.lin,
                              node_weight=b.node_weight.copy())
        getattr(c, f)[0] *= 2.0
        with pytest.raises(ValueError):
            models.potts_node_weight_groups([a, c])
    assert len(models.potts_node_weight_groups([a, b])[1]) == 2


class _NoSampler:
    """Fails the test if the driver reaches the sampler."""

    def sample_dqm_many(self, *args, **kwargs):
        raise AssertionError("the driver reached the sampler")


@pytest.mark.parametrize("resolutions", [[], (0.5, 0.5), (0.5, 0.0), (-1.0,), (0.5, float("nan")), (float("inf"),)])
def test_sweep_driver_rejects_bad_resolutions(resolutions):
    from scrna_seq_qannealing_clustering_amd import clustering_modularity_sweep
    G = load_fixture("blobs").graph()
    with pytest.raises(ValueError):
        clustering_modularity_sweep(G, resolutions, sampler=_NoSampler())
    with pytest.raises(ValueError):
        models.build_modularity_sweep(G, resolutions)


def test_sample_dqm_many_rejects_mismatched_models():
    from scrna_seq_qannealing_clustering_amd import MI355XSampler
    G = load_fixture("blobs").graph()
    a = models.build_modularity_potts(G, 0.5, 8)
    with pytest.raises(ValueError):                      # checked before any upload
        MI355XSampler(device=0).sample_dqm_many([a, models.build_modularity_potts(G, 1.0, 12)], num_reads=4)
    with pytest.raises(ValueError):
        MI355XSampler(device=0).sample_dqm_many([a, models.build_dqm_potts(G, 8, 0.5)], num_reads=4)


def test_abi_node_weight_groups_rejects_null_handle():
    lib = _lib.load()
    cw = np.zeros(8, dtype=np.float32)
    c64 = np.zeros(2, dtype=np.float64)
    rc = lib.mi_sa_problem_set_node_weight_groups(None, 2, cw.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                  c64.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                  c64.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert rc == -1 and b"NULL" in lib.mi_last_error()
