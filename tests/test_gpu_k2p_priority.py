"""K2p's sweeping wavefronts share their SIMD by a priority that each of them changes once per sweep, derived from its
hardware wave slot and the launch's own sweep index (csrc/sparse_pair_kernels.hip, round 7; the pipelined forms: threshold
wavefront, 16-bit neighbour words, with and without the carried prefetch).  Priority and timing change no value a wavefront
computes, so no test here can tell which priority a sweep ran at; what they pin is that the results stay right: states,
fp64 energies and accepted counts are the oracle's on the device's own order, bit for bit, and the kernel keeps its name.
GPU only.

Shapes: hand-laid models of 64-seat slots without edges inside a slot (recipe of tests/test_gpu_k2p_group_reads.py, copied):
the carried form at 6 slots (n = 384: every seat taken), 7 (4 g + 3) and 9 (4 g + 1), the form without carry at 5; rows
capped at 15 (trimmed) and 16 (full); 2 and 3 replicas (3: the idle seat B of the second wavefront) and 1026 (513
workgroups: more wavefronts than the chip has SIMDs, so sweeping wavefronts share SIMDs); 1, 2 and 9 sweeps (one
priority only, both, and an odd count that ends on the first again)."""
import functools

import numpy as np
import pytest

from oracle import sa_oracle as so
from scrna_seq_qannealing_clustering_amd.engine import Problem

pytestmark = pytest.mark.gpu

SHAPES = [(5, 40), (6, 64), (7, 40), (9, 40)]             # (slots, variables of the last slot); 5: no carry


def f32(x):
    return np.asarray(x, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def slotted_model(slots, cap, last=40, seed=1):
    """A model laid out by hand in `slots` blocks of 64 seats (the last one holds `last` variables): random edges between
    different blocks only, every row at most `cap` entries and the first rows exactly `cap`."""
    rng = np.random.RandomState(seed)
    n = 64 * (slots - 1) + last
    nbrs = [dict() for _ in range(n)]
    deg, block = np.zeros(n, dtype=np.int64), np.arange(n) // 64
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
    assert np.diff(rowptr).max() == cap
    return rowptr, col, val, f32(rng.randn(n)), float(np.float32(0.05))


@functools.lru_cache(maxsize=None)
def oracle_run(slots, last, cap, R, sweeps, seed):
    """the oracle's (states, energies, stats) of a hot-to-cold schedule; computed once per case and only read"""
    args = slotted_model(slots, cap, last)
    return so.sa_csr_rank1_philox(*args, R, np.geomspace(2e-3, 30.0, sweeps), seed)


def pair_name(cap):
    return "k_anneal_csr_rank1_pair<16, tw> r%d" % cap if cap < 16 else "k_anneal_csr_rank1_pair<16, tw>"


def pipelined(p):
    p.set_option("k2_pair", 1)
    p.set_option("k2_tw", 1)
    p.set_option("k2_nbr16", 0)


def fetch_checked(p, cap):
    """what the last anneal left, after making sure that the pipelined pair form ran it (16-bit packing: 6144 bytes per
    slot trimmed, 6400 with full rows)"""
    assert p.kernel_name() == pair_name(cap) and p.adjacency_bytes_per_slot() == (6144 if cap < 16 else 6400)
    return p.fetch()


def check_oracle(got, o, proposals):
    st, en, info = got
    assert np.array_equal(st, o[0])
    assert info["accepted"] == int(o[2][1]) and info["proposals"] == proposals
    print("energies: max |gpu - oracle| / |oracle| = %.3e" % np.max(np.abs(en - o[1]) / np.abs(o[1])))
    assert np.array_equal(en, o[1])


@pytest.mark.parametrize("R", [2, 3])
@pytest.mark.parametrize("sweeps", [1, 2, 9])
@pytest.mark.parametrize("cap", [15, 16])
@pytest.mark.parametrize("slots,last", SHAPES)
def test_rotation_states(slots, last, cap, sweeps, R):
    args = slotted_model(slots, cap, last)
    with Problem.csr_rank1(*args) as p:
        pipelined(p)
        p.anneal(R, np.geomspace(2e-3, 30.0, sweeps), 9)
        check_oracle(fetch_checked(p, cap), oracle_run(slots, last, cap, R, sweeps, 9), R * sweeps * len(args[3]))


@pytest.mark.parametrize("cap", [15, 16])
@pytest.mark.parametrize("slots,last", SHAPES)
def test_many_workgroups(slots, last, cap):
    """1026 replicas: 513 sweeping and 513 threshold wavefronts, so SIMDs hold wavefronts of more than one workgroup and
    sweeping wavefronts run beside each other at priorities that change from sweep to sweep (not observed here: the
    results must be the oracle's whatever the priorities were)."""
    args = slotted_model(slots, cap, last)
    with Problem.csr_rank1(*args) as p:
        pipelined(p)
        p.anneal(1026, np.geomspace(2e-3, 30.0, 9), 13)
        check_oracle(fetch_checked(p, cap), oracle_run(slots, last, cap, 1026, 9, 13), 1026 * 9 * len(args[3]))


@pytest.mark.parametrize("slots,last", [(5, 40), (6, 64)])
def test_one_temperature_per_replica(slots, last):
    args = slotted_model(slots, 15, last)
    rb = np.array([0.05, 1.0, 20.0])
    o = so.sa_csr_rank1_philox(*args, 3, rb, 5, num_sweeps=9)
    with Problem.csr_rank1(*args) as p:
        pipelined(p)
        p.anneal(3, rb, 5, num_sweeps=9)
        check_oracle(fetch_checked(p, 15), o, 3 * 9 * len(args[3]))


@pytest.mark.parametrize("slots,last", [(5, 40), (6, 64), (7, 40)])
def test_continued_launches(slots, last):
    """The rotation counts the sweeps of its own launch, the chain's random stream the sweeps of the run (sweep_offset):
    a schedule cut into launches of 3, 1 and 5 sweeps ends where the single launch ends, which is where the oracle ends."""
    args = slotted_model(slots, 15, last)
    betas = np.geomspace(2e-3, 30.0, 9)
    o = oracle_run(slots, last, 15, 3, 9, 21)
    with Problem.csr_rank1(*args) as p:
        pipelined(p)
        p.anneal(3, betas, 21)
        whole = fetch_checked(p, 15)
        check_oracle(whole, o, 3 * 9 * len(args[3]))
        accepted = 0
        for lo, hi in ((0, 3), (3, 4), (4, 9)):
            p.anneal(3, betas[lo:hi], 21, continue_run=lo > 0, sweep_offset=lo)
            st, en, info = fetch_checked(p, 15)
            accepted += info["accepted"]
        assert np.array_equal(st, o[0]) and np.array_equal(en, whole[1]) and accepted == int(o[2][1])
