"""K2p's 16-bit neighbour words (option k2_nbr16, csrc/sparse_pair_kernels.hip N16): the packed adjacency carries two LDS
addresses per dword, 6144 bytes per slot and wavefront at 16 entries per variable (6400 with full rows, 12544 at 32 entries)
instead of 7936 / 8448 / 16640.  Same chain as the 32-bit packing (k2_nbr16 = 2) and the oracle: states, accepted and
proposal counts bit for bit, fp64 energies to 1e-12; the kernel's name does not depend on the packing, which
`Problem.adjacency_bytes_per_slot()` reports.  The 16-wide form WITHOUT a threshold wavefront (k2_tw = 2) measured slower
with 16-bit words and keeps the 32-bit packing under either option value (profiles/r05_k2p_nbr16_ab.txt).  GPU only.

Shapes: the models of tests/test_gpu_k2p_trim.py (recipe copied) for the row lengths, and hand-laid models of a chosen
number of 64-seat slots -- every edge between two slots, so the layout is taken as it is -- for the exits of the four-slot
trip and the clamp of the two-slots-ahead prefetch (1, 2, 3, 5, 8 slots) and for the highest addresses (72 slots)."""
import functools

import numpy as np
import pytest

import bench
from oracle import sa_oracle as so
from scrna_seq_qannealing_clustering_amd import graphs, models
from scrna_seq_qannealing_clustering_amd.engine import Problem

pytestmark = pytest.mark.gpu


def f32(x):
    return np.asarray(x, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def capped_model(cap, n=1400, seed=5):
    """A synthetic SNN model whose every node has at most `cap` neighbours (edges dropped greedily in edge order)."""
    nodes, eu, ev, w, _ = graphs.synthetic_snn(n, 5, 15, 15, 6, seed=seed, spread=2.5)
    deg = np.zeros(n, dtype=np.int64)
    keep = np.zeros(len(eu), dtype=bool)
    for e, (u, v) in enumerate(zip(eu, ev)):
        if deg[u] < cap and deg[v] < cap:
            keep[e] = True
            deg[u] += 1
            deg[v] += 1
    m = models.build_bqm_qubo(graphs.EdgeListGraph(nodes, eu[keep], ev[keep], w[keep]), 0.05)
    assert np.diff(m.rowptr).max() == cap
    return m


def padded(m):
    pos, nslots, clashes = models.padded_slot_layout(m.rowptr, m.col)
    assert clashes == 0
    N = nslots * 64
    rp, cc, vv = models.pad_csr(m.rowptr, m.col, f32(m.val), pos, N)
    lin = np.full(N, np.inf, dtype=np.float32)
    lin[pos] = f32(m.lin)
    return pos, N, (rp, cc, vv, lin, float(np.float32(m.c_pair)))


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


def run(p, nbr16, R, betas, seed, **kw):
    p.set_option("k2_nbr16", nbr16)
    p.anneal(R, betas, seed, **kw)
    name, nbytes = p.kernel_name(), p.adjacency_bytes_per_slot()
    st, en, info = p.fetch()
    return name, st, en, info, nbytes


def check_same(a, b):
    assert np.array_equal(a[1], b[1])
    assert a[3]["accepted"] == b[3]["accepted"] and a[3]["proposals"] == b[3]["proposals"]
    assert np.allclose(a[2], b[2], rtol=1e-12, atol=0.0)


def pair_name(D, tw, rw):
    if rw:
        return "k_anneal_csr_rank1_pair<%d, tw> r%d" % (D, rw)
    return "k_anneal_csr_rank1_pair<%d, tw>" % D if tw else "k_anneal_csr_rank1_pair<%d>" % D


def wide_bytes(D, rw):
    """the 32-bit packings: D / 4 groups of 2048 bytes and the dword of linear terms; trimmed rows (pack_pair_adjacency)"""
    if rw == 15:
        return 7936
    if rw:
        return 3 * 2048 + (rw - 12) * 512 + 256
    return D * 512 + 256


@pytest.mark.parametrize("cap,trim,tw", [(13, 0, 1), (14, 0, 1), (15, 0, 1), (15, 2, 1), (15, 0, 2)])
def test_row_lengths_match_wide_words_and_oracle(cap, trim, tw):
    """Rows of 13, 14, 15 entries (trimmed: the 6144-byte image, the linear term in the sixteenth value), of 15 with
    trimming off (the full-row image with a padding entry); 15 also without a threshold wavefront."""
    m = capped_model(cap)
    pos, N, oargs = padded(m)
    betas = np.geomspace(2e-3, 30.0, 16)
    o = so.sa_csr_rank1_philox(*oargs, 7, betas, 21)
    rw = cap if (cap < 16 and trim == 0 and tw == 1) else 0
    with Problem.csr_rank1(m.rowptr, m.col, f32(m.val), f32(m.lin), oargs[4], order="padded",
                           energy_model=(m.val, m.lin, m.c_pair)) as p:
        p.set_option("k2_pair", 1)
        p.set_option("k2_tw", tw)
        p.set_option("k2_trim", trim)
        new = run(p, 0, 64, betas, 21)
        old = run(p, 2, 64, betas, 21)
        assert new[0] == old[0] == pair_name(16, tw == 1, rw)
        assert new[4] == (6144 if rw else (6400 if tw == 1 else 8448)) and old[4] == wide_bytes(16, rw)
        check_same(new, old)
        assert np.array_equal(new[1][:7], o[0][:, pos]) and new[3]["accepted"] == old[3]["accepted"]
        assert np.allclose(new[2], m.energies(new[1]), rtol=1e-12)
        assert run(p, 1, 64, betas, 21)[4] == new[4]


@pytest.mark.parametrize("tw", [1, 2])
def test_rows_of_sixteen(tw):
    """A model whose longest row is exactly 16 entries: every half of every neighbour dword is a real address."""
    args = slotted_model(6, 16, seed=4)
    betas = np.geomspace(2e-3, 30.0, 16)
    o = so.sa_csr_rank1_philox(*args, 7, betas, 17)
    with Problem.csr_rank1(*args) as p:
        p.set_option("k2_pair", 1)
        p.set_option("k2_tw", tw)
        new = run(p, 0, 33, betas, 17)
        old = run(p, 2, 33, betas, 17)
        assert new[0] == old[0] == pair_name(16, tw == 1, 0) and (new[4], old[4]) == (6400 if tw == 1 else 8448, 8448)
        check_same(new, old)
        assert np.array_equal(new[1][:7], o[0]) and np.allclose(new[2][:7], o[1], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("slots", [1, 2, 3, 5, 8])
def test_slot_counts(slots):
    """Every exit of the four-slot trip (t + 1 / t + 2 / t + 3 < slots) and the clamp of the prefetch two slots ahead;
    lanes past n in the last slot.  One slot has no edges: the full-row image."""
    args = slotted_model(slots, 15)
    betas = np.geomspace(2e-3, 30.0, 24)
    o = so.sa_csr_rank1_philox(*args, 7, betas, 9)
    with Problem.csr_rank1(*args) as p:
        p.set_option("k2_pair", 1)
        p.set_option("k2_tw", 1)
        new = run(p, 0, 33, betas, 9)
        old = run(p, 2, 33, betas, 9)
        rw = 15 if slots > 1 else 0
        assert new[0] == old[0] == pair_name(16, True, rw)
        assert new[4] == (6144 if rw else 6400) and old[4] == wide_bytes(16, rw)
        check_same(new, old)
        assert np.array_equal(new[1][:7], o[0]) and np.allclose(new[2][:7], o[1], rtol=1e-9, atol=1e-9)
        assert new[3]["proposals"] == 33 * 24 * len(args[3])


def test_highest_addresses():
    """72 slots (4608 seats, the largest model that keeps 16 replicas per CU): bit 14 of the address set in both halves"""
    args = slotted_model(72, 15, last=64, seed=2)
    hi = args[1][args[1] >= 4096]
    assert len(hi) > 100 and len(args[3]) == 4608
    betas = np.geomspace(2e-3, 30.0, 8)
    o = so.sa_csr_rank1_philox(*args, 7, betas, 5)
    with Problem.csr_rank1(*args) as p:
        p.set_option("k2_pair", 1)
        p.set_option("k2_tw", 1)
        new = run(p, 0, 32, betas, 5)
        old = run(p, 2, 32, betas, 5)
        assert new[0] == old[0] == pair_name(16, True, 15) and (new[4], old[4]) == (6144, 7936)
        check_same(new, old)
        assert np.array_equal(new[1][:7], o[0]) and np.allclose(new[2][:7], o[1], rtol=1e-9, atol=1e-9)


def test_call_variants():
    """As tests/test_gpu_k2p_trim.py: a replica offset, given initial states, an odd replica count above 1024, a continued
    run (states + sweep offset) and one temperature per replica, on the padded 15-entry model."""
    m = capped_model(15)
    n = m.num_variables
    pos, N, oargs = padded(m)
    assert N > n                                                          # the layout has holes
    betas = np.geomspace(2e-3, 30.0, 24)
    R = 1101
    init = np.random.RandomState(3).randint(0, 2, size=(R, n)).astype(np.uint8)
    init_dev = np.zeros((7, N), dtype=np.uint8)
    init_dev[:, pos] = init[:7]
    o_rand = so.sa_csr_rank1_philox(*oargs, 7, betas, 21, replica_offset=5)
    o_init = so.sa_csr_rank1_philox(*oargs, 7, betas, 21, init=init_dev)
    o_half = so.sa_csr_rank1_philox(*oargs, 7, betas[:10], 21)
    o_cont = so.sa_csr_rank1_philox(*oargs, 7, betas[10:], 21, init=o_half[0], sweep_offset=10)
    with Problem.csr_rank1(m.rowptr, m.col, f32(m.val), f32(m.lin), oargs[4], order="padded",
                           energy_model=(m.val, m.lin, m.c_pair)) as p:
        p.set_option("k2_pair", 1)
        p.set_option("k2_tw", 1)
        new = run(p, 0, R, betas, 21, replica_offset=5)
        assert new[0] == "k_anneal_csr_rank1_pair<16, tw> r15" and new[4] == 6144
        old = run(p, 2, R, betas, 21, replica_offset=5)
        assert old[0] == new[0] and old[4] == 7936
        check_same(new, old)
        assert np.array_equal(new[1][:7], o_rand[0][:, pos]) and np.allclose(new[2], m.energies(new[1]), rtol=1e-12)
        # given initial states
        new = run(p, 0, R, betas, 21, initial_states=init)
        check_same(new, run(p, 2, R, betas, 21, initial_states=init))
        assert np.array_equal(new[1][:7], o_init[0][:, pos])
        # continuation: 10 sweeps, then the rest from the states left on the device
        for nbr16 in (0, 2):
            p.set_option("k2_nbr16", nbr16)
            p.anneal(R, betas[:10], 21)
            p.anneal(R, betas[10:], 21, continue_run=True, sweep_offset=10)
            assert p.adjacency_bytes_per_slot() == (6144 if nbr16 == 0 else 7936)
            st, en, info = p.fetch()
            assert np.array_equal(st[:7], o_cont[0][:, pos]) and np.allclose(en, m.energies(st), rtol=1e-12)
            if nbr16 == 0:
                first = (None, st, en, info)
            else:
                check_same(first, (None, st, en, info))
        # one temperature per replica
        rb = np.geomspace(0.05, 20.0, R)
        new = run(p, 0, R, rb, 21, num_sweeps=12)
        assert new[0].endswith(" r15") and new[4] == 6144
        check_same(new, run(p, 2, R, rb, 21, num_sweeps=12))
        o_pr = so.sa_csr_rank1_philox(*oargs, 7, rb[:7], 21, num_sweeps=12)
        assert np.array_equal(new[1][:7], o_pr[0][:, pos])


@pytest.mark.parametrize("cap,slots", [(17, 2), (30, 3), (32, 8)])
def test_32_entries(cap, slots):
    """The 32-wide layout (no threshold wavefront, two blocks of sixteen gathers per slot): 12544 bytes against 16640."""
    args = slotted_model(slots, cap, seed=3)
    betas = np.geomspace(2e-3, 30.0, 16)
    o = so.sa_csr_rank1_philox(*args, 7, betas, 13)
    with Problem.csr_rank1(*args) as p:
        p.set_option("k2_pair", 1)
        new = run(p, 0, 33, betas, 13)
        old = run(p, 2, 33, betas, 13)
        assert new[0] == old[0] == "k_anneal_csr_rank1_pair<32>" and (new[4], old[4]) == (12544, 16640)
        check_same(new, old)
        assert np.array_equal(new[1][:7], o[0]) and np.allclose(new[2][:7], o[1], rtol=1e-9, atol=1e-9)


def test_other_kernels_report_no_packing():
    """One replica per wavefront (k2_pair = 2): a kernel without such a packing reports 0 bytes."""
    args = slotted_model(3, 15)
    with Problem.csr_rank1(*args) as p:
        p.set_option("k2_pair", 2)
        p.set_option("k2_split", 2)
        p.anneal(16, np.geomspace(0.1, 10.0, 4), 1)
        assert "pair" not in p.kernel_name() and p.adjacency_bytes_per_slot() == 0


def test_bench_model_default():
    """The benchmark's model at its replica count: the default kernel reads the 16-bit packing (6144 bytes) under its
    unchanged name, and runs the chain of the 32-bit packing and of the oracle."""
    m = bench.build_workload()[0]
    assert np.diff(m.rowptr).max() == 15
    pos, N, oargs = padded(m)
    betas = models.make_beta_schedule(30, models.default_beta_range(m))
    o = so.sa_csr_rank1_philox(*oargs, 4, betas, 77)
    with Problem.csr_rank1(m.rowptr, m.col, f32(m.val), f32(m.lin), oargs[4], order="padded",
                           energy_model=(m.val, m.lin, m.c_pair)) as p:
        p.anneal(4096, betas, 77)                                          # no option set: the library's own choice
        assert p.kernel_name() == "k_anneal_csr_rank1_pair<16, tw> r15" and p.adjacency_bytes_per_slot() == 6144
        new = run(p, 0, 4096, betas, 77)
        old = run(p, 2, 4096, betas, 77)
        assert new[0] == old[0] == "k_anneal_csr_rank1_pair<16, tw> r15" and (new[4], old[4]) == (6144, 7936)
        check_same(new, old)
        assert np.array_equal(new[1][:4], o[0][:, pos]) and new[3]["proposals"] == 4096 * 30 * m.num_variables
        assert np.allclose(new[2], m.energies(new[1]), rtol=1e-12)
