"""tests/chain_ends_reference.py -- the reported energy of a structured anneal restated in float64 loops -- against the
host's fp64 evaluation of the same models, without a GPU.

On every model of tests/chain_ends_cases.py the reference on random states agrees with ``models.QuboModel.energies`` /
``models.PottsModel.energies`` (numpy sums of the same coefficients in another order) to rtol = 1e-12 -- for K2s' 1, 2
and 4 wavefronts too; with one wavefront, one lane's worth of data and c_pair = 0 it IS a straight sequential sum,
bit for bit (the butterfly then only adds zeros)."""
import numpy as np
import pytest

import chain_ends_cases as cc
import chain_ends_reference as ref
from scrna_seq_qannealing_clustering_amd import models


def _qubo(m, offset):
    """The host model of the coefficients the device sums (fp32 values widened, or the fp64 energy model)."""
    if m.spec.f64:
        val, lin, c = m.val64, m.lin64, m.c64
    else:
        val, lin, c = m.val.astype(np.float64), m.lin.astype(np.float64), m.c_pair
    return models.QuboModel(list(range(m.n)), lin, m.rowptr, m.col, val, c_pair=c, offset=offset, weights=m.weights)


@pytest.mark.parametrize("name", sorted(cc.BINARY))
def test_binary_reference_agrees_with_the_host_model(name):
    m = cc.model(name)
    X = np.random.RandomState(1).randint(0, 2, size=(4, m.n)).astype(np.uint8)
    X[0] = 0
    X[1] = 1
    want = _qubo(m, 0.75).energies(X)
    # (K2s with 2 or 4 wavefronts takes whole groups of four slots: the layouts in blocks of 128 / 256 seats)
    wave_counts = (1, 2, 4) if (m.n_dev // 64) % 4 == 0 else (1,)
    assert len(wave_counts) == 3 or m.spec.block == 64
    for waves in wave_counts:
        got = ref.binary_energies(m.to_device(X, np.uint8), *cc.binary_reference_args(m), offset=0.75, weights=m.d_weights,
                                  waves=waves)
        assert np.allclose(got, want, rtol=1e-12, atol=0.0)
        assert got[0] == 0.75


@pytest.mark.parametrize("name", sorted(cc.POTTS))
@pytest.mark.parametrize("K", [2, 9, 16, 64])
def test_potts_reference_agrees_with_the_host_model(name, K):
    m = cc.model(name)
    L = np.random.RandomState(2).randint(0, K, size=(3, m.n)).astype(np.uint16)
    L[0] = 0
    pm = models.PottsModel(list(range(m.n)), K, m.rowptr, m.col, m.val.astype(np.float64), m.c_pair, np.full(m.n, 0.25))
    got = ref.potts_energies(m.to_device(L, np.uint16), m.d_rowptr, m.d_col, m.d_val, m.c_pair, pm.lin_offset, K, present=m.present)
    assert np.allclose(got, pm.energies(L), rtol=1e-12, atol=0.0)
    # node weights, two resolution groups: the group's pair coefficient and offset
    wq, cw, w64, c64, offset = cc.node_weights(m)
    nw = np.zeros(m.n_dev)
    nw[m.seats] = w64
    for g in range(2):
        pm = models.PottsModel(list(range(m.n)), K, m.rowptr, m.col, m.val.astype(np.float64), float(c64[g]),
                               np.full(m.n, offset[g] / m.n), node_weight=w64)
        got = ref.potts_energies(m.to_device(L, np.uint16), m.d_rowptr, m.d_col, m.d_val, c64[g], offset[g], K, nw64=nw)
        assert np.allclose(got, pm.energies(L), rtol=1e-12, atol=0.0)


def test_butterfly_of_one_lane_is_that_lane():
    v = [0.0] * 64
    v[0] = 0.1 + 0.2
    assert ref.butterfly(v) == 0.1 + 0.2
    assert ref.butterfly([1.0] * 64) == 64.0


def test_one_lane_is_a_sequential_sum():
    """Only the variables of lane 0 (positions 0, 64, 128, ...) are on and c_pair = 0: every other lane's partial is +0.0,
    the butterfly adds zeros, and the energy is the plain loop over lane 0's slots."""
    m = cc.model("hub70")                                            # caller's order, c_pair = 0, a row of 70 at variable 0
    assert m.c_pair == 0.0 and m.n_dev == m.n
    x = np.zeros(m.n, dtype=np.uint8)
    x[::64] = 1
    on = set(range(0, m.n, 64))
    e = 0.0
    for i in sorted(on):
        acc = 0.0
        for k in range(m.rowptr[i], m.rowptr[i + 1]):
            if m.col[k] in on:
                acc += float(m.val[k])
        e += float(m.lin[i]) + 0.5 * acc
    assert ref.binary_energy(x, m.d_rowptr, m.d_col, m.d_val, m.d_lin, 0.0) == e + 0.0 * 0.5 * 0.0 + 0.0
    assert e != 0.0
