"""K2p's trimmed rows (`k_anneal_csr_rank1_pair<16, tw> r<RW>`, csrc/sparse_pair_kernels.hip): models whose longest row
has RW = 13..15 entries at the 16-wide layout skip the padding entries RW..15 (neither fetched nor gathered).  Same chain
as the untrimmed kernel (option k2_trim = 2) and the oracle: states and accepted counts bit for bit, fp64 energies to
1e-12.  GPU only."""
import numpy as np
import pytest

import bench
from oracle import sa_oracle as so
from scrna_seq_qannealing_clustering_amd import graphs, models
from scrna_seq_qannealing_clustering_amd.engine import Problem

pytestmark = pytest.mark.gpu


def f32(x):
    return np.asarray(x, dtype=np.float32)


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


def run(p, trim, R, betas, seed, **kw):
    p.set_option("k2_trim", trim)
    p.anneal(R, betas, seed, **kw)
    name = p.kernel_name()
    st, en, info = p.fetch()
    return name, st, en, info


def check_same(a, b):
    assert np.array_equal(a[1], b[1])
    assert a[3]["accepted"] == b[3]["accepted"] and a[3]["proposals"] == b[3]["proposals"]
    assert np.allclose(a[2], b[2], rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("cap", [15, 14, 13])
def test_trimmed_rows_match_untrimmed_and_oracle(cap):
    """Odd and even RW below 16 on a padded layout (holes): random and given initial states, a replica offset, an odd
    replica count, a continued run (states + sweep offset) and one temperature per replica."""
    m = capped_model(cap)
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
        tr = run(p, 0, R, betas, 21, replica_offset=5)
        assert tr[0] == "k_anneal_csr_rank1_pair<16, tw> r%d" % cap
        full = run(p, 2, R, betas, 21, replica_offset=5)
        assert full[0] == "k_anneal_csr_rank1_pair<16, tw>"
        check_same(tr, full)
        assert np.array_equal(tr[1][:7], o_rand[0][:, pos]) and np.allclose(tr[2], m.energies(tr[1]), rtol=1e-12)
        assert run(p, 1, R, betas, 21, replica_offset=5)[0] == tr[0]
        # given initial states
        tr = run(p, 0, R, betas, 21, initial_states=init)
        check_same(tr, run(p, 2, R, betas, 21, initial_states=init))
        assert np.array_equal(tr[1][:7], o_init[0][:, pos])
        # continuation: 10 sweeps, then the rest from the states left on the device
        for trim in (0, 2):
            p.set_option("k2_trim", trim)
            p.anneal(R, betas[:10], 21)
            p.anneal(R, betas[10:], 21, continue_run=True, sweep_offset=10)
            st, en, info = p.fetch()
            assert np.array_equal(st[:7], o_cont[0][:, pos]) and np.allclose(en, m.energies(st), rtol=1e-12)
            if trim == 0:
                first = (None, st, en, info)
            else:
                check_same(first, (None, st, en, info))
        # one temperature per replica
        rb = np.geomspace(0.05, 20.0, R)
        tr = run(p, 0, R, rb, 21, num_sweeps=12)
        assert tr[0].endswith(" r%d" % cap)
        check_same(tr, run(p, 2, R, rb, 21, num_sweeps=12))
        o_pr = so.sa_csr_rank1_philox(*oargs, 7, rb[:7], 21, num_sweeps=12)
        assert np.array_equal(tr[1][:7], o_pr[0][:, pos])


def test_trimmed_rows_on_the_bench_model():
    """The benchmark's model (maximum degree 15 at the 16-wide layout): its default K2p kernel is the trimmed one, and
    it runs the untrimmed kernel's chain."""
    m = bench.build_workload()[0]
    assert np.diff(m.rowptr).max() == 15
    pos, N, oargs = padded(m)
    betas = models.make_beta_schedule(30, models.default_beta_range(m))
    o = so.sa_csr_rank1_philox(*oargs, 4, betas, 77)
    with Problem.csr_rank1(m.rowptr, m.col, f32(m.val), f32(m.lin), oargs[4], order="padded",
                           energy_model=(m.val, m.lin, m.c_pair)) as p:
        tr = run(p, 0, 4096, betas, 77)
        assert tr[0] == "k_anneal_csr_rank1_pair<16, tw> r15"
        full = run(p, 2, 4096, betas, 77)
        assert full[0] == "k_anneal_csr_rank1_pair<16, tw>"
        check_same(tr, full)
        assert np.array_equal(tr[1][:4], o[0][:, pos]) and tr[3]["proposals"] == 4096 * 30 * m.num_variables
        assert np.allclose(tr[2], m.energies(tr[1]), rtol=1e-12)

