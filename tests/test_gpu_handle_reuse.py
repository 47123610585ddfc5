"""One handle used again at other sizes computes what a fresh handle computes: the device buffers a handle owns are sized
per call (replicas, sweeps, initial states, tempering ladders, resolution groups, selected genes), and every path that
regrows one is run here on a handle that has already served another size.  Trajectories are frozen per seed and replica
offset, so a reused handle and a fresh one agree exactly."""
import subprocess
import sys

import numpy as np
import pytest

from scrna_seq_qannealing_clustering_amd import preprocess, umap
from scrna_seq_qannealing_clustering_amd.engine import Problem

pytestmark = pytest.mark.gpu

N_SLOT = 130                     # three 64-variable slots, the last one partial
K = 4


def sparse_model(seed, n=N_SLOT, degree=6):
    """A symmetric CSR with both directions stored, no diagonal, about `degree` neighbours per row."""
    rs = np.random.default_rng(seed)
    A = np.zeros((n, n), dtype=np.float32)
    for i in range(n):
        for j in rs.choice(n, size=degree // 2, replace=False):
            if i != j:
                A[i, j] = A[j, i] = np.float32(rs.normal())
    rowptr = np.zeros(n + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum((A != 0).sum(axis=1))
    col = np.concatenate([np.nonzero(A[i])[0] for i in range(n)]).astype(np.int32)
    val = np.concatenate([A[i][np.nonzero(A[i])[0]] for i in range(n)]).astype(np.float32)
    return rowptr, col, val, rs


def make_dense(n, seed):
    rs = np.random.default_rng(seed)
    Q = rs.normal(size=(n, n)).astype(np.float32)
    return np.ascontiguousarray((Q + Q.T) * np.float32(0.5))


_XL = {}


def dense_xl_matrix():
    if "Q" not in _XL:
        _XL["Q"] = make_dense(4160, 5)          # the smallest n padded to two 4096-column chunks
    return _XL["Q"]


def new_problem(kind, options=()):
    if kind == "dense":
        p = Problem.dense(make_dense(100, 3))
    elif kind == "dense_xl":
        p = Problem.dense(dense_xl_matrix())
    elif kind == "csr_rank1":
        rowptr, col, val, rs = sparse_model(11)
        p = Problem.csr_rank1(rowptr, col, val, rs.normal(size=N_SLOT).astype(np.float32), 0.02)
    else:
        rowptr, col, val, _ = sparse_model(12)
        p = Problem.potts_csr(rowptr, col, val, 0.03, N_SLOT, K)
    for key, value in options:
        p.set_option(key, value)
    return p


def schedule(sweeps):
    return np.geomspace(0.2, 4.0, sweeps)


# ---- 1. an anneal handle across replica counts, sweep counts and initial states ---------------------------------------

@pytest.mark.parametrize("kind,options,R", [
    ("dense", (), 64),
    ("dense_xl", (("xl_batched", 1), ("xl_async", 0)), 4),      # the cooling run of 40 sweeps in the caller
    ("dense_xl", (("xl_batched", 1), ("xl_async", 1)), 4),      # ... and in the problem's worker thread (the default)
    ("csr_rank1", (), 64),
    ("potts", (), 64),
])
def test_problem_reused_across_sizes_equals_fresh_problems(kind, options, R):
    """R replicas x 8 sweeps; 3 R x 40 sweeps from given initial states (states, energies, initial states and
    temperatures regrow); R x 8 again; 8 more sweeps continued.  Every step equals the same call(s) on a fresh handle."""
    n = {"dense": 100, "dense_xl": 4160}.get(kind, N_SLOT)
    rs = np.random.default_rng(21)
    dtype = np.uint16 if kind == "potts" else np.uint8
    init = rs.integers(0, K if kind == "potts" else 2, size=(3 * R, n)).astype(dtype)
    steps = [                                                           # (steps run on a fresh handle, the one compared)
        [dict(num_reads=R, betas=schedule(8), seed=101)],
        [dict(num_reads=3 * R, betas=schedule(40), seed=102, replica_offset=7, initial_states=init)],
        [dict(num_reads=R, betas=schedule(8), seed=103, replica_offset=2)],
        [dict(num_reads=R, betas=schedule(8), seed=103, replica_offset=2),
         dict(num_reads=R, betas=schedule(8)[::-1].copy(), seed=103, replica_offset=2, sweep_offset=8, continue_run=True)],
    ]
    reused = []
    with new_problem(kind, options) as p:
        for calls in steps:
            p.anneal(**calls[-1])
            st, en, _ = p.fetch()
            reused.append((st.copy(), en.copy()))
            if kind == "dense_xl":                                      # (the batched kernels: 40 sweeps are a cooling run)
                assert "k_xg" in p.kernel_name(), p.kernel_name()
    for calls, (st, en) in zip(steps, reused):
        with new_problem(kind, options) as q:
            for call in calls:
                q.anneal(**call)
            st1, en1, _ = q.fetch()
        assert st.shape == (calls[-1]["num_reads"], n)
        assert np.array_equal(st, st1) and np.array_equal(en, en1)
    assert not np.array_equal(reused[0][0], reused[2][0])               # (the steps are different runs)


def test_dense_plan_does_not_depend_on_what_the_handle_ran_before():
    """Forced K1w at n = 64 with launches of 2 sweeps: 40 replicas x 5 sweeps are cut into 3 launches and leave the buffer of
    cached fields allocated; 19 replicas on the same handle are then one launch of the same kernel, as on a fresh handle
    (fewer than 32 replicas are never cut), and the states are the oracle's."""
    from oracle import sa_oracle as so
    Qs, betas, options = make_dense(64, 17), schedule(5), (("variant", 2), ("chunk_sweeps", 2))

    def run(p, R):
        p.anneal(R, betas, 31, replica_offset=3)
        st, _, info = p.fetch()
        return p.kernel_name(), p.launch_count(), st, info["accepted"]

    with Problem.dense(Qs) as fresh:
        for key, value in options:
            fresh.set_option(key, value)
        want = run(fresh, 19)
    with Problem.dense(Qs) as p:
        for key, value in options:
            p.set_option(key, value)
        assert run(p, 40)[:2] == ("k_anneal_dense_wg<4,4>", 3)
        got = run(p, 19)
    assert got[:2] == want[:2] == ("k_anneal_dense_wg<4,4>", 1)
    ost, _, ostats = so.sa_dense_philox(Qs, 19, betas, 31, replica_offset=3)
    assert np.array_equal(got[2], ost) and np.array_equal(want[2], ost) and got[3] == want[3] == int(ostats[1])


# ---- 2. tempering set up twice ---------------------------------------------------------------------------------------

def tempering_round(p, T, chains, seed):
    R = T * chains
    p.tempering_begin(np.geomspace(0.3, 5.0, T), chains, 0, R)
    p.anneal(R, None, seed, num_sweeps=3)
    p.tempering_exchange(0, seed + 1)
    rung, proposed, accepted = p.tempering_state()
    st, en, _ = p.fetch()
    return rung, proposed, accepted, st, en


def test_tempering_set_up_again_equals_a_fresh_setup():
    with new_problem("potts") as p:
        first = tempering_round(p, 4, 5, 31)
        again = tempering_round(p, 6, 7, 41)
    with new_problem("potts") as q:
        fresh = tempering_round(q, 6, 7, 41)
    assert first[0].shape == (20,) and again[0].shape == (42,)
    assert again[1] == fresh[1] > 0 and again[2] == fresh[2]
    for a, b in zip(again, fresh):
        assert np.array_equal(a, b)


# ---- 3. resolution groups set twice before the first anneal ----------------------------------------------------------

def group_tables(G, seed):
    rs = np.random.default_rng(seed)
    cw = rs.uniform(0.001, 0.01, size=(G, N_SLOT)).astype(np.float32)
    return cw, rs.uniform(0.01, 0.05, size=G), rs.normal(size=G)


def test_groups_set_again_equal_a_fresh_problem():
    rs = np.random.default_rng(51)
    wq = rs.integers(1, 9, size=N_SLOT).astype(np.int32)
    cw0 = (wq * np.float32(0.002)).astype(np.float32)
    results = []
    for first in (3, None):
        with new_problem("potts") as p:
            p.set_node_weights(wq, cw0)
            if first:
                p.set_node_weight_groups(*group_tables(first, 52))
            p.set_node_weight_groups(*group_tables(2, 53))
            p.anneal(6, schedule(10), 61)
            st, en, _ = p.fetch()
            results.append((st, en))
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    assert not np.array_equal(results[0][1][:3], results[0][1][3:])       # (two groups, two objectives)


# ---- 4. a UMAP graph built twice on one handle -----------------------------------------------------------------------

def test_umap_graph_built_again_equals_the_first():
    X = np.random.default_rng(71).normal(size=(130, 5)).astype(np.float32)
    with umap.FuzzyGraph(X, 4) as g:
        first = g.smooth().union().fetch_graph()
        info = g.info()
        again = g.smooth().union().fetch_graph()
        assert g.info() == info and info["nnz"] == len(first[1]) > 0
    for a, b in zip(first, again):
        assert np.array_equal(a, b)


# ---- 5. a prep matrix scaled at two widths ---------------------------------------------------------------------------

def test_pca_at_two_widths_equals_fresh_matrices():
    X = np.random.default_rng(81).poisson(1.5, size=(90, 200)).astype(np.float32)
    widths = (np.arange(40), np.arange(5, 175))                         # 128 and 256 padded columns: the second regrows
    with preprocess.ExpressionMatrix(X) as m:
        m.normalize()
        reused = [preprocess.pca(m, genes, npcs=5) for genes in widths]
    for genes, r in zip(widths, reused):
        with preprocess.ExpressionMatrix(X) as f:
            f.normalize()
            fresh = preprocess.pca(f, genes, npcs=5)
        assert r.coords.shape == (90, 5)
        assert np.array_equal(r.coords, fresh.coords) and np.array_equal(r.eigenvalues, fresh.eigenvalues)


# ---- 6. destroy right after create, and after a refused setter -------------------------------------------------------

_DESTROY = r"""
import ctypes as C
import numpy as np
from scrna_seq_qannealing_clustering_amd import _lib, preprocess, umap
from scrna_seq_qannealing_clustering_amd.engine import Problem
from test_gpu_handle_reuse import new_problem
lib = _lib.load()
EINVAL = -1
for refuse in (False, True):
    for kind in ("dense", "dense_xl", "csr_rank1", "potts"):
        p = new_problem(kind)
        if refuse:
            assert lib.mi_sa_set_option(p._h, b"no_such_option", 1) == EINVAL
            assert lib.mi_sa_problem_set_merge_moves(p._h, -1, 1, None) == EINVAL
        assert lib.mi_sa_problem_destroy(p._h) == 0
        p._h = None
    m = preprocess.ExpressionMatrix(np.ones((4, 3), dtype=np.float32))
    if refuse:
        assert lib.mi_prep_normalize(m._h, C.c_double(-1.0), None) == EINVAL
    assert lib.mi_prep_destroy(m._h) == 0
    m._h = None
    X = np.random.default_rng(1).normal(size=(20, 3)).astype(np.float32)
    g = umap.FuzzyGraph(X, 4)
    assert lib.mi_umap_destroy(g._h) == 0
    g._h = None
    h = C.c_void_p()
    assert lib.mi_snn_build_f32(X.ctypes.data_as(C.POINTER(C.c_float)), 20, 3, 4, 0.0, 0, 0, C.byref(h)) == 0
    assert lib.mi_snn_destroy(h) == 0
print("clean")
"""


def test_destroy_right_after_create_and_after_a_refused_setter():
    """Each of the four handle types destroyed without having been used, and the handles that have a setter with
    arguments to refuse (the problem, the prep matrix) destroyed after one answered MI_EINVAL: MI_OK, and the process
    (a child of its own, so that its end is seen) ends clean."""
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]))
    run = subprocess.run([sys.executable, "-c", _DESTROY], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stdout.strip() == "clean", run.stdout + run.stderr
