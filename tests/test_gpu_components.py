"""Batched connected components on the GPU (mi_graph_components, mi_sa_problem_components, csrc/components_kernels.hip)
against ``scipy.sparse.csgraph.connected_components`` on the filtered graph, renumbered by smallest cell ascending.  The
result is a pure function of the input, so every comparison is integer equality, in both forms of the kernel (parent array
in LDS, and in HBM through the ``MI_COMPONENTS_GLOBAL`` flag), which must also agree with each other: long paths in and
against the index order (an iteration cap or plain label propagation would stop short), degenerate graphs, random sparse
graphs at the sizes where the wavefront and the scan chunk end, per-item label and keep filters, a keep mask set in one
stored direction only, the reference's fixtures; the in-place pass over a padded-layout Potts anneal; the sampler's
``split_disconnected=True`` and the drivers."""
import ctypes as C

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components as scipy_components

from conftest import load_fixture
from test_gpu_modularity import graph, problem
from scrna_seq_qannealing_clustering_amd import _lib, clustering, graphs, metrics, models
from scrna_seq_qannealing_clustering_amd.engine import Problem
from scrna_seq_qannealing_clustering_amd.sampler import MI355XSampler, default_potts_beta_range, model_edges

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -6
RTOL = 1e-9                                   # the project's fp64 energy tolerance


def ref_components(n, eu, ev, live=None):
    """scipy on the live edges; components renumbered 0 .. C - 1 by their smallest cell, ascending"""
    eu, ev = np.asarray(eu), np.asarray(ev)
    if live is not None:
        eu, ev = eu[live], ev[live]
    A = coo_matrix((np.ones(len(eu), dtype=np.int8), (eu, ev)), shape=(n, n))
    nc, lab = scipy_components(A, directed=False)
    first = np.full(nc, n, dtype=np.int64)
    np.minimum.at(first, lab, np.arange(n))
    rank = np.empty(nc, dtype=np.int64)
    rank[np.argsort(first)] = np.arange(nc)
    return rank[lab].astype(np.int32), nc


def ref_batch(n, eu, ev, L=None, keep=None):
    """one scipy call per item: edge e is live when its ends carry one label and keep[b, e] is set"""
    B = len(L) if L is not None else (len(keep) if keep is not None else 1)
    labs, cnts = [], []
    for b in range(B):
        live = np.ones(len(eu), dtype=bool)
        if L is not None:
            live &= L[b][eu] == L[b][ev]
        if keep is not None:
            live &= keep[b] != 0
        lab, nc = ref_components(n, eu, ev, live)
        labs.append(lab)
        cnts.append(nc)
    return np.stack(labs), np.asarray(cnts, dtype=np.int32)


def csr_one_direction(n, eu, ev):
    order = np.argsort(eu, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(eu, minlength=n))]).astype(np.int32)
    return rowptr, np.ascontiguousarray(np.asarray(ev)[order], dtype=np.int32), order


def raw(rowptr, col, n, L=None, keep=None, flags=0, B=None, rc=False):
    """the C ABI; outputs pre-filled with -7"""
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
    col = np.ascontiguousarray(col, dtype=np.int32)
    L = None if L is None else np.ascontiguousarray(L, dtype=np.uint16)
    keep = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)
    if B is None:
        B = len(L) if L is not None else (len(keep) if keep is not None else 1)
    out = np.full((max(B, 1), n), -7, dtype=np.int32)
    cnt = np.full(max(B, 1), -7, dtype=np.int32)
    i32p = C.POINTER(C.c_int32)
    ptr = (lambda a, t: None if a is None else a.ctypes.data_as(t))
    ms = C.c_float(-1.0)
    code = _lib.load().mi_graph_components(rowptr.ctypes.data_as(i32p), col.ctypes.data_as(i32p), n, ptr(L, C.POINTER(C.c_uint16)),
                                           ptr(keep, C.POINTER(C.c_uint8)), B, 0, flags, out.ctypes.data_as(i32p),
                                           cnt.ctypes.data_as(i32p), C.byref(ms))
    if rc:
        return code
    _lib.check(code)
    assert ms.value >= 0.0
    return out, cnt


def both_forms(rowptr, col, n, L=None, keep=None):
    """the LDS form and the forced global form: identical arrays"""
    a, ca = raw(rowptr, col, n, L, keep, 0)
    g, cg = raw(rowptr, col, n, L, keep, 1)
    assert np.array_equal(a, g) and np.array_equal(ca, cg)
    return a, ca


def check(n, eu, ev, L=None, keep=None):
    """edges stored once, keep per edge: both forms against scipy"""
    rowptr, col, order = csr_one_direction(n, eu, ev)
    out, cnt = both_forms(rowptr, col, n, L, None if keep is None else np.asarray(keep)[:, order])
    want, wcnt = ref_batch(n, np.asarray(eu), np.asarray(ev), L, keep)
    assert np.array_equal(cnt, wcnt)
    assert np.array_equal(out, want)
    return out, cnt


# ---- 1. long paths: no iteration cap, no O(diameter) propagation cut short ---------------------------------------------

def path_edges(order):
    return np.asarray(order[:-1], dtype=np.int32), np.asarray(order[1:], dtype=np.int32)


def test_path_of_1001_cells():
    n = 1001
    eu, ev = path_edges(np.arange(n))
    out, cnt = check(n, eu, ev)
    assert cnt[0] == 1 and not out.any()


def test_path_renumbered_by_a_permutation():
    n = 1001
    order = np.random.default_rng(1001).permutation(n)
    eu, ev = path_edges(order)
    out, cnt = check(n, eu, ev)
    assert cnt[0] == 1 and not out.any()
    out, cnt = check(n, ev, eu)                                    # the stored direction reversed
    assert cnt[0] == 1


@pytest.mark.parametrize("permute", [False, True])
def test_path_with_labels_in_blocks_of_7(permute):
    n = 1001
    order = np.random.default_rng(7).permutation(n) if permute else np.arange(n)
    eu, ev = path_edges(order)
    L = np.empty((1, n), dtype=np.int64)
    L[0, order] = np.arange(n) // 7                                # the label follows the position along the path
    out, cnt = check(n, eu, ev, L)
    assert cnt[0] == -(-n // 7) == 143
    assert np.array_equal(np.bincount(out[0]), np.bincount(L[0]))  # same block sizes (7 ... 7)


# ---- 2. degenerate graphs -------------------------------------------------------------------------------------------------

def test_single_cell_and_no_edges():
    out, cnt = check(1, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
    assert out.tolist() == [[0]] and cnt.tolist() == [1]
    out, cnt = check(130, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
    assert cnt[0] == 130 and np.array_equal(out[0], np.arange(130))
    out, cnt = check(1, np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32))     # one cell with a self loop
    assert out.tolist() == [[0]] and cnt.tolist() == [1]


@pytest.mark.parametrize("centre", [0, 199, 77])
def test_star(centre):
    n = 200
    leaves = np.array([i for i in range(n) if i != centre], dtype=np.int32)
    out, cnt = check(n, np.full(n - 1, centre, dtype=np.int32), leaves)
    assert cnt[0] == 1
    L = (np.arange(n) % 2)[None, :]                                # the centre keeps every second leaf
    out, cnt = check(n, leaves, np.full(n - 1, centre, dtype=np.int32), L)
    assert cnt[0] == 1 + (n - 1) - int(np.sum(L[0][leaves] == L[0][centre]))


def test_isolated_cells_among_connected_ones_and_self_loops():
    n = 130
    rng = np.random.default_rng(130)
    alone = np.array([3, 64, 65, 100, 129])
    rest = np.setdiff1d(np.arange(n), alone)
    perm = rng.permutation(rest)
    eu = np.concatenate([perm[:-1], rng.choice(rest, 60)])
    ev = np.concatenate([perm[1:], rng.choice(rest, 60)])         # a spanning path plus chords (some are self loops)
    out, cnt = check(n, eu, ev)
    assert cnt[0] == 6 and np.bincount(out[0]).max() == 125
    # a self loop on every cell: connects nothing
    out2, cnt2 = check(n, np.concatenate([eu, np.arange(n)]), np.concatenate([ev, np.arange(n)]))
    assert np.array_equal(out, out2) and cnt2[0] == 6


# ---- 3. random sparse graphs, per-item filters ------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [63, 64, 65, 257, 2638])
@pytest.mark.parametrize("B", [1, 3, 64])
def test_random_graphs_labels_and_keep(n, B):
    rng = np.random.default_rng(n * 131 + B)
    m = (3 * n) // 2                                               # mean degree 3: many components
    eu, ev = rng.integers(0, n, m).astype(np.int32), rng.integers(0, n, m).astype(np.int32)
    assert ref_components(n, eu, ev)[1] > 1
    for K in (2, 16):
        L = rng.integers(0, K, (B, n))
        check(n, eu, ev, L)                                        # labels only
        keep = rng.random((B, m)) < 0.7
        out, cnt = check(n, eu, ev, L, keep)                       # labels and a keep mask
        assert np.all(cnt == out.max(axis=1) + 1)
    check(n, eu, ev, None, rng.random((B, m)) < 0.6)               # a keep mask only
    # both directions stored, the keep mask set in ONE stored direction of each kept edge: it must still connect
    su, sv = np.concatenate([eu, ev]), np.concatenate([ev, eu])
    kept = rng.random((B, m)) < 0.6
    side = rng.random((B, m)) < 0.5
    keep2 = np.concatenate([kept & side, kept & ~side], axis=1)
    rowptr, col, order = csr_one_direction(n, su, sv)
    L = rng.integers(0, 2, (B, n))
    for lab in (None, L):
        out, cnt = both_forms(rowptr, col, n, lab, keep2[:, order])
        want, wcnt = ref_batch(n, eu, ev, lab, kept)
        assert np.array_equal(out, want) and np.array_equal(cnt, wcnt)


def test_python_entry_forms_agree():
    """(eu, ev), an (m, 2) array and (rowptr, col); 1-D labels; labels outside uint16 compacted; force_global"""
    n, m = 257, 380
    rng = np.random.default_rng(5)
    eu, ev = rng.integers(0, n, m).astype(np.int32), rng.integers(0, n, m).astype(np.int32)
    L = rng.integers(0, 5, (3, n))
    keep = rng.random((3, m)) < 0.7
    want, wcnt = ref_batch(n, eu, ev, L, keep)
    rowptr, col, order = csr_one_direction(n, eu, ev)
    for g, k in (((eu, ev), keep), (np.stack([eu, ev], axis=1), keep), ((rowptr, col), keep[:, order])):
        for fg in (False, True):
            out, cnt = metrics.connected_components(g, n, labels=L, keep=k, force_global=fg)
            assert out.dtype == np.int32 and np.array_equal(out, want) and np.array_equal(cnt, wcnt)
    one, c1 = metrics.connected_components((eu, ev), n, labels=L[1])
    assert one.shape == (1, n) and np.array_equal(one[0], ref_batch(n, eu, ev, L[1:2])[0][0])
    far, cf = metrics.split_disconnected((eu, ev), n, L * 100003 - 7)              # labels outside uint16
    assert np.array_equal(far, ref_batch(n, eu, ev, L)[0])
    plain, cp = metrics.connected_components((eu, ev), n)
    assert plain.shape == (1, n) and np.array_equal(plain[0], ref_components(n, eu, ev)[0])
    assert np.array_equal(metrics.connected_components((eu, ev), n, keep=keep[0])[0][0], ref_batch(n, eu, ev, None, keep[:1])[0][0])


# ---- 4. the reference's fixtures ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,sizes", [("noisy_circles", [128, 128]), ("blobs", [86, 85, 85]), ("noisy_moons", [256]),
                                        ("varied", [256]), ("aniso", [256]), ("no_structure", [256])])
def test_fixture_components(name, sizes):
    f = load_fixture(name)
    n = len(f.nodes)
    out, cnt = check(n, f.eu, f.ev, np.zeros((1, n), dtype=np.int64))
    assert cnt[0] == len(sizes)
    assert sorted(np.bincount(out[0]).tolist(), reverse=True) == sizes
    split, sc = metrics.split_disconnected((f.eu, f.ev), n, np.zeros(n, dtype=np.int64))
    assert np.array_equal(split, out) and np.array_equal(sc, cnt)


# ---- 5. the global form at its natural size -----------------------------------------------------------------------------

def test_renumbered_path_just_above_the_lds_limit():
    n = metrics.COMPONENTS_LDS_MAX_CELLS + 1
    order = np.random.default_rng(n).permutation(n)
    eu, ev = path_edges(order)
    rowptr, col, _ = csr_one_direction(n, eu, ev)
    out, cnt = raw(rowptr, col, n)                                 # no flag: the size alone selects the form
    assert cnt[0] == 1 and not out.any()
    L = np.empty((2, n), dtype=np.int64)
    L[0, order] = np.arange(n) // 1000
    L[1, order] = np.arange(n) // 4097
    out, cnt = metrics.connected_components((eu, ev), n, labels=L)
    want, wcnt = ref_batch(n, eu, ev, L)
    assert np.array_equal(cnt, wcnt) and cnt.tolist() == [27, 7] and np.array_equal(out, want)
    # ... and the LDS form at the limit itself
    n = metrics.COMPONENTS_LDS_MAX_CELLS
    order = np.random.default_rng(n).permutation(n)
    eu, ev = path_edges(order)
    L = np.empty((1, n), dtype=np.int64)
    L[0, order] = np.arange(n) // 1000
    check(n, eu, ev, L)


# ---- 6. in place: the states and the adjacency of a padded-layout Potts problem --------------------------------------

def smoke_graph():
    nodes, eu, ev, ww, _ = graphs.synthetic_snn(900, 5, 15, 15, 5, seed=4, spread=2.5)
    return graphs.EdgeListGraph(nodes, eu, ev, ww)


def padded_run(interrupted):
    pm = models.build_modularity_potts(smoke_graph(), 1.0, 16)
    betas = models.make_beta_schedule(40, default_potts_beta_range(pm))
    with problem(pm, order="padded") as p:
        n = pm.num_variables
        assert p.n_dev > n and not np.array_equal(np.asarray(p._inv), np.arange(n))    # holes, seats not the identity
        p.anneal(24, betas[:20], 7)
        mid = mid_states = after = None
        if interrupted:
            mid_states = p.fetch()[0]
            mid = p.components()
            after = p.fetch()[0]
        p.anneal(24, betas[20:], 7, sweep_offset=20, continue_run=True)
        st, en, _ = p.fetch()
        end = p.components()
    return pm, st, en, mid_states, mid, after, end


def test_problem_components_matches_host_and_leaves_the_run():
    pm, st, en, mid_states, mid, after, end = padded_run(True)
    _, st0, en0, _, _, _, end0 = padded_run(False)
    assert np.array_equal(mid_states, after)                        # fetch() before and after
    assert np.array_equal(st, st0) and np.array_equal(en, en0)      # the continued run equals the uninterrupted one
    n = pm.num_variables
    eu, ev = model_edges(pm)
    for states, (lab, cnt) in ((mid_states, mid), (st, end), (st0, end0)):
        host, hcnt = metrics.connected_components((pm.rowptr, pm.col), n, labels=states)
        assert lab.shape == (24, n) and lab.dtype == np.int32
        assert np.array_equal(lab, host) and np.array_equal(cnt, hcnt)
        want, wcnt = ref_batch(n, eu, ev, states)
        assert np.array_equal(lab, want) and np.array_equal(cnt, wcnt)
    assert np.any(mid[1] > [len(np.unique(r)) for r in mid_states])   # an early state has disconnected clusters


def test_problem_components_raw_holes_and_errors():
    pm = models.build_modularity_potts(graph("s16"), 1.0, 8)
    lib = _lib.load()
    i32p = C.POINTER(C.c_int32)
    with problem(pm, order="padded") as p:
        with pytest.raises(RuntimeError):
            p.components()
        nd = p.n_dev
        out = np.full((4, nd), -7, dtype=np.int32)
        cnt = np.full(4, -7, dtype=np.int32)
        assert lib.mi_sa_problem_components(p._h, out.ctypes.data_as(i32p), cnt.ctypes.data_as(i32p), None) == ESTATE
        p.anneal(4, models.make_beta_schedule(10, default_potts_beta_range(pm)), 3)
        assert lib.mi_sa_problem_components(p._h, None, cnt.ctypes.data_as(i32p), None) == EINVAL
        _lib.check(lib.mi_sa_problem_components(p._h, out.ctypes.data_as(i32p), cnt.ctypes.data_as(i32p), None))
        holes = np.ones(nd, dtype=bool)
        holes[np.asarray(p._inv)] = False
        assert holes.any() and np.all(out[:, holes] == -1) and np.all(out[:, ~holes] >= 0)   # hole seats are not cells
        assert np.array_equal(cnt, out.max(axis=1) + 1)
        lab, c2 = p.components()
        assert np.array_equal(c2, cnt)
        for r in range(4):                                            # the same partition, numbered in the caller's order
            assert np.array_equal(metrics.renumber_by_first_cell(out[r:r + 1][:, np.asarray(p._inv)])[0], lab[r])
    with Problem.dense(np.eye(8, dtype=np.float32)) as d:
        d.anneal(4, np.ones(3), 1)
        assert lib.mi_sa_problem_components(d._h, out.ctypes.data_as(i32p), cnt.ctypes.data_as(i32p), None) == ESTATE


# ---- 7. sampler and drivers ---------------------------------------------------------------------------------------------

SPLIT_KEYS = {"split_labels", "split_num_clusters", "split_energy", "split_modularity"}


def check_split(ss, pm, f):
    """the split entries of a sampleset's info: refinement, connectivity, energies"""
    n = len(f.nodes)
    samples = np.asarray(ss.record["sample"])
    energy = np.asarray(ss.record["energy"])
    split, k2, e2 = ss.info["split_labels"], ss.info["split_num_clusters"], ss.info["split_energy"]
    assert split.shape == samples.shape and split.dtype == np.int32 and len(k2) == len(e2) == len(samples)
    want, wcnt = ref_batch(n, f.eu, f.ev, samples)
    assert np.array_equal(split, want) and np.array_equal(k2, wcnt)
    for r in range(len(samples)):
        k1 = len(np.unique(samples[r]))
        pairs = np.unique(np.stack([split[r], samples[r]]), axis=1)
        assert pairs.shape[1] == k2[r]                              # every split cluster inside one original label
        conn, nconn = ref_batch(n, f.eu, f.ev, split[r:r + 1])
        assert nconn[0] == k2[r]                                    # every split cluster is connected
        tol = RTOL * max(abs(energy[r]), abs(e2[r]))
        print("record %d: clusters %d -> %d, energy %.17g -> %.17g" % (r, k1, k2[r], energy[r], e2[r]))
        assert e2[r] <= energy[r] + tol
        assert (abs(e2[r] - energy[r]) <= tol) == (k2[r] == k1)     # equal exactly where the count did not change
    assert np.array_equal(e2, models.potts_energies_any(pm, split))
    return split


def test_sampler_split_lifts_the_cluster_cap_and_changes_nothing_else():
    f = load_fixture("blobs")
    G = f.graph()
    kw = dict(num_reads=16, num_sweeps=60, seed=3)
    plain = clustering.clustering_modularity(G, 1.0, 2, sampler_kwargs=kw)
    ss = clustering.clustering_modularity(G, 1.0, 2, sampler_kwargs=kw, split_disconnected=True)
    assert list(ss.variables) == f.nodes
    for key in ("sample", "energy", "num_occurrences"):
        assert np.array_equal(plain.record[key], ss.record[key]), key
    assert set(ss.info) - set(plain.info) == SPLIT_KEYS and not (SPLIT_KEYS & set(plain.info))
    pm = models.build_modularity_potts(G, 1.0, 2)
    check_split(ss, pm, f)
    assert np.all(ss.info["split_num_clusters"] >= 3)             # three blobs under two labels: the cap is lifted
    assert np.all(ss.info["split_modularity"] >= ss.info["modularity"] - RTOL * np.abs(ss.info["modularity"]))
    assert np.array_equal(ss.info["split_modularity"], -ss.info["split_energy"] / pm.info["m"])
    # the DQM driver and the plain sampler entry
    dq = clustering.clustering_dqm(G, 2, 0.005, sampler_kwargs=kw, split_disconnected=True)
    dq0 = clustering.clustering_dqm(G, 2, 0.005, sampler_kwargs=kw)
    assert np.array_equal(dq.record["sample"], dq0.record["sample"]) and np.array_equal(dq.record["energy"], dq0.record["energy"])
    assert set(dq.info) - set(dq0.info) == SPLIT_KEYS - {"split_modularity"}
    check_split(dq, models.build_dqm_potts(G, 2, 0.005), f)
    assert np.all(dq.info["split_num_clusters"] >= 3)


def test_sweep_split_and_consensus_from_one_call():
    f = load_fixture("blobs")
    G = f.graph()
    n = len(f.nodes)
    kw = dict(num_reads=16, num_sweeps=60, seed=3)
    res = [0.5, 1.0, 2.0]
    sets = clustering.clustering_modularity_sweep(G, res, 2, consensus=True, split_disconnected=True, sampler_kwargs=kw)
    plain = clustering.clustering_modularity_sweep(G, res, 2, consensus=True, sampler_kwargs=kw)
    pms = models.build_modularity_sweep(G, res, 2)
    for ss, pl, pm in zip(sets, plain, pms):
        for key in ("sample", "energy", "num_occurrences"):
            assert np.array_equal(pl.record[key], ss.record[key]), key
        assert set(ss.info) - set(pl.info) == SPLIT_KEYS
        eu, ev = ss.info["consensus_edges"]
        host = metrics.consensus_labels(ss.info["edge_cooccurrence"], 1, eu, ev, n, 0.5)     # (a share: of 1 read)
        assert np.array_equal(ss.info["consensus_labels"], host)
        assert np.array_equal(pl.info["consensus_labels"], host)
        split, cnt = metrics.split_disconnected((pm.rowptr, pm.col), n, np.asarray(ss.record["sample"]))
        assert np.array_equal(ss.info["split_labels"], split) and np.array_equal(ss.info["split_num_clusters"], cnt)
        check_split(ss, pm, f)
        one = clustering.clustering_modularity(G, pm.info["resolution"], 2, split_disconnected=True, sampler_kwargs=kw)
        for key in SPLIT_KEYS:
            assert np.array_equal(one.info[key], ss.info[key]), key
