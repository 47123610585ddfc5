"""K2p's fixed costs per group, per sweep and per launch (csrc/sparse_pair_kernels.hip, round 6), on the pipelined form
(threshold wavefront, 16-bit neighbour words):
  * the lane's own cells and the thresholds of a group of four slots are read once, at the top of the group (pair reads
    256 bytes apart; in a last group of one to three slots the missing slots' reads are clamped into the cell array);
  * in sweeps of six slots and more the adjacency prefetch is carried over the end of a sweep (the prefetch index wraps;
    4 g + 1 and 4 g + 3 slots end a sweep in the other register set), below six every sweep fills its own pipeline;
  * the fp64 energy epilogue requests a slot's indices and values together (both value types: fp64 from an energy model,
    fp32 from the model itself).
Same chain as the oracle: states, accepted and proposal counts bit for bit (every replica is run by the oracle as well),
fp64 energies to 1e-12 relative.  GPU only.

Shapes: hand-laid models of 1 .. 9 slots of 64 seats, the last one 40 wide (recipe of tests/test_gpu_k2p_nbr16.py, copied):
every residue of slots % 4 on both sides of the carry threshold.  2 or 3 replicas (3: the idle seat B of the second
wavefront), rows capped at 13, 15 and 16 entries."""
import functools

import numpy as np
import pytest

from oracle import sa_oracle as so
from scrna_seq_qannealing_clustering_amd.engine import Problem

pytestmark = pytest.mark.gpu


def f32(x):
    return np.asarray(x, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def slotted_model(slots, cap, last=40, seed=1):
    """A model laid out by hand in `slots` blocks of 64 seats (the last one holds `last` variables): random edges between
    different blocks only, every row at most `cap` entries and the first rows exactly `cap` (none with one block)."""
    rng = np.random.RandomState(seed)
    n = 64 * (slots - 1) + last
    nbrs = [dict() for _ in range(n)]
    deg, block = np.zeros(n, dtype=np.int64), np.arange(n) // 64
    if slots > 1:
        for i in range(n):
            free = np.flatnonzero((block != block[i]) & (deg < cap))
            for j in rng.permutation(free)[:cap]:
                if deg[i] < cap and int(j) not in nbrs[i]:
                    nbrs[i][int(j)] = nbrs[j][i] = np.float32(rng.randn())
                    deg[i] += 1
                    deg[j] += 1
    rowptr = np.zeros(n + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum([len(d) for d in nbrs])
    col = np.array([j for d in nbrs for j in sorted(d)], dtype=np.int32)
    val = np.array([d[j] for d in nbrs for j in sorted(d)], dtype=np.float32)
    assert np.diff(rowptr).max() == (cap if slots > 1 else 0)
    return rowptr, col, val, f32(rng.randn(n)), float(np.float32(0.05))


def pair_name(rw):
    return "k_anneal_csr_rank1_pair<16, tw> r%d" % rw if rw else "k_anneal_csr_rank1_pair<16, tw>"


def packed_bytes(rw):
    """the 16-bit packings (pack_pair_adjacency16): two blocks of neighbour dwords and four of values; full rows carry
    the dword of linear terms besides"""
    return 6144 if rw else 6400


def pipelined(p):
    p.set_option("k2_pair", 1)
    p.set_option("k2_tw", 1)
    p.set_option("k2_nbr16", 0)


def fetch_checked(p, rw):
    """what the last anneal left, after making sure that the pipelined pair form ran it"""
    assert p.kernel_name() == pair_name(rw) and p.adjacency_bytes_per_slot() == packed_bytes(rw)
    return p.fetch()


def check_oracle(got, o, proposals):
    st, en, info = got
    assert np.array_equal(st, o[0])
    assert info["accepted"] == int(o[2][1]) and info["proposals"] == proposals
    assert np.allclose(en, o[1], rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("R", [2, 3])
@pytest.mark.parametrize("sweeps", [1, 5])
@pytest.mark.parametrize("slots", [1, 2, 3, 4, 5, 6, 7, 8, 9])
def test_slot_counts(slots, sweeps, R):
    """One sweep crosses no sweep boundary, five cross four.  One slot has no edges: the full-row image."""
    args = slotted_model(slots, 15)
    betas = np.geomspace(2e-3, 30.0, sweeps)
    o = so.sa_csr_rank1_philox(*args, R, betas, 9)
    with Problem.csr_rank1(*args) as p:
        pipelined(p)
        p.anneal(R, betas, 9)
        check_oracle(fetch_checked(p, 15 if slots > 1 else 0), o, R * sweeps * len(args[3]))


@pytest.mark.parametrize("cap", [13, 15, 16])
@pytest.mark.parametrize("slots", [6, 7])
def test_row_caps_hot_to_cold(slots, cap):
    """Two trimmed forms and full rows, 40 sweeps from hot to cold: slots that accept and slots that accept nothing."""
    args = slotted_model(slots, cap, seed=4)
    betas = np.geomspace(2e-3, 30.0, 40)
    o = so.sa_csr_rank1_philox(*args, 3, betas, 17)
    hot = so.sa_csr_rank1_philox(*args, 3, betas[:20], 17)
    # (the hot half accepts most of the run's moves: the cold half has slots that accept nothing)
    assert 0 < int(o[2][1]) - int(hot[2][1]) < int(hot[2][1]) // 2
    with Problem.csr_rank1(*args) as p:
        pipelined(p)
        p.anneal(3, betas, 17)
        check_oracle(fetch_checked(p, cap if cap < 16 else 0), o, 3 * 40 * len(args[3]))


@pytest.mark.parametrize("slots", [6, 7])
def test_schedule_cut_into_launches(slots):
    """A structured anneal is one launch, so the cut is made by continuing the run (states left on the device, the random
    stream by sweep_offset): three launches give the single launch's result bit for bit -- nothing of the carried prefetch
    outlives a launch."""
    args = slotted_model(slots, 15)
    betas = np.geomspace(2e-3, 30.0, 12)
    o = so.sa_csr_rank1_philox(*args, 3, betas, 21)
    with Problem.csr_rank1(*args) as p:
        pipelined(p)
        p.anneal(3, betas, 21)
        assert p.launch_count() == 1
        whole = fetch_checked(p, 15)
        check_oracle(whole, o, 3 * 12 * len(args[3]))
        launches, accepted = 0, 0
        for lo, hi in ((0, 5), (5, 6), (6, 12)):
            p.anneal(3, betas[lo:hi], 21, continue_run=lo > 0, sweep_offset=lo)
            launches += p.launch_count()
            st, en, info = fetch_checked(p, 15)
            accepted += info["accepted"]
        assert launches > 1
        assert np.array_equal(st, whole[0]) and np.array_equal(en, whole[1]) and accepted == whole[2]["accepted"]


def test_given_initial_states():
    args = slotted_model(6, 15)
    betas = np.geomspace(0.5, 30.0, 5)
    init = np.random.RandomState(3).randint(0, 2, size=(3, len(args[3]))).astype(np.uint8)
    o = so.sa_csr_rank1_philox(*args, 3, betas, 5, init=init)
    with Problem.csr_rank1(*args) as p:
        pipelined(p)
        p.anneal(3, betas, 5, initial_states=init)
        check_oracle(fetch_checked(p, 15), o, 3 * 5 * len(args[3]))


def test_one_temperature_per_replica():
    args = slotted_model(6, 15)
    rb = np.array([0.05, 1.0, 20.0])
    o = so.sa_csr_rank1_philox(*args, 3, rb, 5, num_sweeps=6)
    with Problem.csr_rank1(*args) as p:
        pipelined(p)
        p.anneal(3, rb, 5, num_sweeps=6)
        check_oracle(fetch_checked(p, 15), o, 3 * 6 * len(args[3]))


class Energies:
    """E(x) = sum_i lin_i x_i + 1/2 sum_ij val_ij x_i x_j + c_pair * C(sum x, 2) in fp64, from the CSR arrays"""

    def __init__(self, rowptr, col, val, lin, c_pair):
        self.rows = np.repeat(np.arange(len(lin)), np.diff(rowptr))
        self.col, self.val, self.lin, self.c = col, np.asarray(val, np.float64), np.asarray(lin, np.float64), float(c_pair)

    def energies(self, states):
        x = states.astype(np.float64)
        pair = (x[:, self.rows] * x[:, self.col] * self.val).sum(axis=1)
        s = x.sum(axis=1)
        return x @ self.lin + 0.5 * pair + self.c * s * (s - 1.0) / 2.0


@pytest.mark.parametrize("slots,cap", [(7, 15), (5, 16)])
@pytest.mark.parametrize("with_model", [True, False])
def test_energy_epilogue_both_value_types(slots, cap, with_model):
    """With an energy model the epilogue sums its fp64 values (here NOT the fp32 ones widened: they carry digits below
    fp32's), without one the fp32 values; either way the energies are those of the model evaluated on the host."""
    rowptr, col, val, lin, c = slotted_model(slots, cap, seed=6)
    rng = np.random.RandomState(8)
    val64 = val.astype(np.float64) * (1.0 + 1e-9 * rng.randn(len(val)))
    for i in range(len(lin)):                                             # (keep it symmetric: the entry (j, i) of (i, j))
        for e in range(rowptr[i], rowptr[i + 1]):
            j = col[e]
            if j > i:
                val64[rowptr[j] + np.searchsorted(col[rowptr[j]:rowptr[j + 1]], i)] = val64[e]
    lin64 = lin.astype(np.float64) * (1.0 + 1e-9 * rng.randn(len(lin)))
    c64 = float(c) * (1.0 + 1e-9)
    betas = np.geomspace(2e-3, 30.0, 8)
    o = so.sa_csr_rank1_philox(rowptr, col, val, lin, c, 3, betas, 31)
    kw = dict(energy_model=(val64, lin64, c64)) if with_model else {}
    m = Energies(rowptr, col, val64, lin64, c64) if with_model else Energies(rowptr, col, val, lin, c)
    with Problem.csr_rank1(rowptr, col, val, lin, c, **kw) as p:
        pipelined(p)
        p.anneal(3, betas, 31)
        st, en, info = fetch_checked(p, cap if cap < 16 else 0)
        assert np.array_equal(st, o[0]) and info["accepted"] == int(o[2][1])
        assert np.allclose(en, m.energies(st), rtol=1e-12, atol=0.0)
        if not with_model:
            assert np.allclose(en, o[1], rtol=1e-12, atol=0.0)
