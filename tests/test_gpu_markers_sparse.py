"""The rank-sum marker pass on a resident ``ExpressionMatrix`` (mi_prep_rank_sum_markers, csrc/markers_kernels.hip), sparse
(the CSC kernels: no transpose, no n x g buffer) and dense (the dense kernels on the resident matrix), against the CPU
reference of tests/markers_reference.py on the densified matrix and against the dense entry point
(``metrics.rank_sum_pass`` on an ndarray), which every output must equal bit for bit.  Integers are compared with
``np.array_equal``; every case runs in the LDS form and in the forced HBM form, and on a sparse handle with both ways of
reading the values, which must all equal each other.  The CSR inputs are built as ``csr_matrix((data, indices, indptr))``
so that stored zeros survive."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import prep_reference as ref
from markers_reference import reference_stats, sparse_matrix
from scrna_seq_qannealing_clustering_amd import _lib, metrics, preprocess
from scrna_seq_qannealing_clustering_amd.preprocess import ExpressionMatrix

pytestmark = pytest.mark.gpu

RTOL = 1e-9                                   # the project's fp64 tolerance (tests/test_gpu_markers.py)
CAP = metrics.MARKERS_LDS_MAX_NONZEROS
CHUNK = metrics.MARKERS_LABELLING_CHUNK
EINVAL, ESTATE, EUNSUPPORTED = -1, -6, -5
KEYS = ("rank2", "npos", "tie", "sum")


def csr_of(X, pattern=None):
    """``csr_matrix((data, indices, indptr))`` holding X at the True places of ``pattern`` (default: its non-zeros); a zero
    of X at such a place is a stored zero, with its sign"""
    pattern = (X != 0) if pattern is None else pattern
    rows, cols = np.nonzero(pattern)                                # row-major: the columns of a row ascend
    indptr = np.concatenate([[0], np.cumsum(pattern.sum(axis=1))]).astype(np.int64)
    A = sp.csr_matrix((X[rows, cols].astype(np.float32), cols.astype(np.int32), indptr), shape=X.shape)
    assert A.nnz == int(pattern.sum()) and A.has_canonical_format
    return A


def same(a, b, what):
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), "%s: %s" % (what, key)


def check_handle(m, X, L, K, want, dense_entry, which="counts", plain=False):
    """every form of the pass on the handle ``m`` against the reference integers ``want`` and, on all four outputs, against
    the dense entry point's result; -> the unforced result"""
    forms = [dict(force_global=False), dict(force_global=True)]
    if m.sparse:
        forms += [dict(gather="inplace"), dict(gather="permute"), dict(force_global=True, gather="inplace"),
                  dict(force_global=True, gather="permute")]
    out = []
    for kw in forms:
        r = m.rank_sum_pass(L, K, which=which, plain=plain, **kw)
        assert r["rank2"].shape == (np.asarray(L).reshape(-1, X.shape[0]).shape[0], X.shape[1], K)
        assert np.array_equal(r["rank2"], want[0]), "rank2 %s" % kw
        assert np.array_equal(r["npos"], want[1]), "npos %s" % kw
        assert np.array_equal(r["tie"], want[3]), "tie %s" % kw
        same(r, dense_entry, "dense entry point, %s" % kw)
        out.append(r)
    for r in out[1:]:
        same(out[0], r, "between forms")
    return out[0]


def check_both_handles(X, L, K, pattern=None, plain=False):
    """a sparse and a dense handle of X (``which="counts"``) against the reference and the dense entry point"""
    L = np.asarray(L).reshape(-1, X.shape[0])
    want = reference_stats(X, L, K, plain=plain)
    entry = metrics.rank_sum_pass(X, L, K, plain=plain)
    with ExpressionMatrix(csr_of(X, pattern)) as m:
        assert m.sparse
        before = m.device_bytes()
        r = check_handle(m, X, L, K, want, entry, plain=plain)
        assert m.device_bytes() == before and "markers_ms" in m.timing
    with ExpressionMatrix(X) as m:
        assert not m.sparse
        before = m.device_bytes()
        same(r, check_handle(m, X, L, K, want, entry, plain=plain), "dense handle")
        assert m.device_bytes() == before
    return r, want


# ---- 1. wavefront, workgroup and tile edges -----------------------------------------------------------------------------

@pytest.mark.parametrize("g", [1, 63, 65])
@pytest.mark.parametrize("n", [2, 63, 64, 65, 257])
def test_edges(n, g):
    rng = np.random.default_rng(1000 * n + g)
    X = sparse_matrix(rng, n, g)
    check_both_handles(X, rng.integers(0, 3, (2, n)), 3)


# ---- 2. special genes ---------------------------------------------------------------------------------------------------

def special_genes(rng, n=300):
    """-> names, X (n x genes), pattern of the stored entries"""
    cols, stored = {}, {}

    def add(name, values, pattern):
        cols[name], stored[name] = np.asarray(values, dtype=np.float32), np.asarray(pattern, dtype=bool)

    add("no_entry", np.zeros(n), np.zeros(n))
    add("all_stored_zeros", np.where(rng.random(n) < 0.5, -0.0, 0.0), np.ones(n))
    v = np.where(rng.random(n) < 0.3, rng.uniform(0.5, 3.0, n), np.where(rng.random(n) < 0.5, -0.0, 0.0))
    v[:4] = [-0.0, 0.0, 1.5, 1.5]
    add("mixed_zeros", v, (v != 0) | (rng.random(n) < 0.5) | (np.arange(n) < 4))
    add("every_cell", rng.uniform(0.5, 3.0, n), np.ones(n))
    add("one_tie_group", np.full(n, 1.25), np.ones(n))
    add("all_distinct", rng.permutation(n) + 1.0, np.ones(n))
    for k in (255, 256, 257):
        c = np.zeros(n)
        c[rng.permutation(n)[:k]] = rng.uniform(0.1, 2.0, k)
        add("nonzeros_%d" % k, c, c != 0)
    for k in (256, 257):                                            # k stored entries, one of them a zero: k - 1 non-zeros
        c = np.zeros(n)
        at = rng.permutation(n)[:k]
        c[at[1:]] = np.round(rng.uniform(0.1, 2.0, k - 1), 1)
        p = np.zeros(n, dtype=bool)
        p[at] = True
        add("stored_%d_one_zero" % k, c, p)
    names = list(cols)
    return names, np.stack([cols[k] for k in names], axis=1), np.stack([stored[k] for k in names], axis=1)


def test_special_genes():
    rng = np.random.default_rng(2)
    n = 300
    names, X, P = special_genes(rng, n)
    at = names.index
    stored, nonzero = P.sum(axis=0), (X != 0).sum(axis=0)
    assert stored[at("no_entry")] == 0
    assert stored[at("all_stored_zeros")] == n and nonzero[at("all_stored_zeros")] == 0
    z = X[P[:, at("mixed_zeros")], at("mixed_zeros")]
    assert (z != 0).any() and np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()
    assert stored[at("every_cell")] == nonzero[at("every_cell")] == n
    assert [int(nonzero[at("nonzeros_%d" % k)]) for k in (255, 256, 257)] == [255, 256, 257]
    # 256 stored, 255 non-zero: both pad to 256; 257 stored, 256 non-zero: planned for 512, the true count would pad to 256
    assert [(int(stored[at("stored_%d_one_zero" % k)]), int(nonzero[at("stored_%d_one_zero" % k)])) for k in (256, 257)] == \
        [(256, 255), (257, 256)]
    L = rng.integers(0, 5, (3, n))
    r, _ = check_both_handles(X, L, 5, pattern=P)
    assert r["tie"][at("all_stored_zeros")] == r["tie"][at("no_entry")] == r["tie"][at("one_tie_group")] == n ** 3 - n
    assert r["tie"][at("all_distinct")] == 0
    assert (r["rank2"].sum(axis=2) == n * (n + 1)).all()            # whatever the labelling
    # an empty cell: row 7 without entries
    X[7], P[7] = 0.0, False
    A = csr_of(X, P)
    assert A.indptr[8] == A.indptr[7]
    r, _ = check_both_handles(X, L, 5, pattern=P)
    assert r["tie"][at("one_tie_group")] == (n - 1) ** 3 - (n - 1) and (r["rank2"].sum(axis=2) == n * (n + 1)).all()


# ---- 3. labellings -------------------------------------------------------------------------------------------------------

def test_one_cluster_and_one_labelling():
    rng = np.random.default_rng(3)
    X = sparse_matrix(rng, 130, 9)
    r, _ = check_both_handles(X, np.zeros(130, dtype=int), 1)        # K = 1, B = 1
    assert (r["rank2"] == 130 * 131).all()


def test_64_clusters_with_unused_labels():
    rng = np.random.default_rng(4)
    X = sparse_matrix(rng, 200, 7)
    L = rng.choice([0, 5, 31, 62, 63], (2, 200))
    r, _ = check_both_handles(X, L, 64)
    unused = np.setdiff1d(np.arange(64), [0, 5, 31, 62, 63])
    assert not r["rank2"][:, :, unused].any() and not r["npos"][:, :, unused].any() and not r["sum"][:, :, unused].any()


def test_one_more_labelling_than_the_chunk_with_a_repeated_row():
    rng = np.random.default_rng(5)
    n = 150
    X = sparse_matrix(rng, n, 11)
    L = rng.integers(0, 6, (CHUNK + 1, n))
    L[CHUNK] = L[0]
    r, _ = check_both_handles(X, L, 6)
    for key in ("rank2", "npos", "sum"):
        assert np.array_equal(r[key][CHUNK], r[key][0]), key


# ---- 4. the LDS cap ------------------------------------------------------------------------------------------------------

def test_lds_cap_in_one_call():
    rng = np.random.default_rng(7)
    n = CAP + 16
    X, P = np.zeros((n, 4), dtype=np.float32), np.zeros((n, 4), dtype=bool)
    # the last LDS gene, the first HBM gene, an HBM gene by its stored count with CAP true non-zeros, a sparse one
    for j, (stored, zeros) in enumerate(((CAP, 0), (CAP + 1, 0), (CAP + 1, 1), (10, 0))):
        at = rng.permutation(n)[:stored]
        P[at, j] = True
        X[at[zeros:], j] = np.round(rng.uniform(0.1, 3.0, stored - zeros), 2)       # (two decimals: ties among the non-zeros)
    assert P.sum(axis=0).tolist() == [CAP, CAP + 1, CAP + 1, 10] and (X != 0).sum(axis=0).tolist() == [CAP, CAP + 1, CAP, 10]
    check_both_handles(X, rng.integers(0, 4, (2, n)), 4, pattern=P)


# ---- 5. the sums ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [2, CHUNK + 1])
def test_sums(B):
    rng = np.random.default_rng(8 + B)
    n, g, K = 257, 65, 5
    X = sparse_matrix(rng, n, g)
    P = (X != 0) | (rng.random(X.shape) < 0.1)                      # some stored zeros
    L = rng.integers(0, K, (B, n))
    r, want = check_both_handles(X, L, K, pattern=P)                # expm1: bit-equal to the dense entry point (inside)
    assert np.allclose(r["sum"], want[2], rtol=RTOL, atol=0.0)
    with ExpressionMatrix(csr_of(X, P)) as m:
        assert np.array_equal(m.rank_sum_pass(L, K, which="counts")["sum"], r["sum"])          # run to run
        assert np.array_equal(m.rank_sum_pass(L, K, which="counts")["sum"], r["sum"])
    r, want = check_both_handles(X, L, K, pattern=P, plain=True)
    assert np.array_equal(r["sum"], want[2])                        # the same additions in the same order


# ---- 6. the normalised chain ---------------------------------------------------------------------------------------------

def test_normalised_chain():
    rng = np.random.default_rng(11)
    n, g = 257, 65
    X = ref.sparse_counts(rng, n, g, rate=0.3)
    A = csr_of(X, (X != 0) | (rng.random(X.shape) < 0.05))
    lab = rng.integers(0, 4, (2, n)) * 3 - 1                         # arbitrary ids
    want = metrics.find_all_markers(preprocess.log_normalize(X), lab)
    fields = [k for k in want if k != "kernel_ms"]
    assert {"U", "p_val", "p_val_adj", "pct_1", "pct_2", "avg_log2FC", "auc", "passed", "cluster_size"} <= set(fields)

    def equal(got, what):
        for key in fields:
            assert np.array_equal(got[key], want[key], equal_nan=True), "%s: %s" % (what, key)

    with ExpressionMatrix(A) as m:
        m.normalize()
        Y = m.fetch_normalized()
        before = m.device_bytes()
        equal(metrics.find_all_markers(m, lab), "sparse handle")
        equal(metrics.find_all_markers(m, lab, which="normalized"), "sparse handle, which")
        assert m.device_bytes() == before
        Y2 = m.fetch_normalized()
        assert np.array_equal(Y2.data, Y.data) and np.array_equal(Y2.indices, Y.indices)
        # the counts are still there, and are what which="counts" ranks
        same(m.rank_sum_pass(lab[0] // 3 + 1, 4, which="counts"), metrics.rank_sum_pass(X, lab[0] // 3 + 1, 4), "counts")
    with ExpressionMatrix(X) as m:
        equal(metrics.find_all_markers(m.normalize(), lab), "dense handle")
    Ys = preprocess.log_normalize(A)
    assert sp.issparse(Ys)
    equal(metrics.find_all_markers(Ys, lab), "log_normalize(csr)")
    one = metrics.find_all_markers(Ys, lab[1], genes=["g%d" % j for j in range(g)])
    assert one["U"].shape == (g, len(one["cluster_ids"])) and one["genes"][3] == "g3"


# ---- 7. beyond the dense limits ------------------------------------------------------------------------------------------

def test_beyond_the_dense_limits():
    """n = 70 000 x g = 65 536 > 2^32 entries, about 2e5 of them stored: no dense handle, no n x g buffer"""
    n, g, B, K = 70000, 65536, 2, 4
    one, handle = np.zeros(1, dtype=np.float32), C.c_void_p()
    assert _lib.load().mi_prep_create_f32(one.ctypes.data_as(C.POINTER(C.c_float)), n, g, 0, C.byref(handle)) == EUNSUPPORTED
    rng = np.random.default_rng(6)
    nnz = 200000
    rows, cols = rng.integers(0, n, nnz), rng.integers(0, g, nnz)
    cols[:3000] = 12345                                             # one dense gene ...
    rows[0], cols[0] = n - 1, 0                                      # ... gene 0 and gene g - 1 have a cell past 65 536
    rows[1], cols[1] = 65536, g - 1
    A = sp.coo_matrix((rng.integers(1, 6, nnz).astype(np.float32), (rows, cols)), shape=(n, g)).tocsr()
    A.sum_duplicates()
    L = rng.integers(0, K, (B, n))
    sizes = np.stack([np.bincount(row, minlength=K) for row in L])
    with ExpressionMatrix(A) as m:
        before = m.device_bytes()
        r = m.rank_sum_pass(L, K, which="counts")
        same(r, m.rank_sum_pass(L, K, which="counts", force_global=True), "HBM form")
        assert m.device_bytes() == before
    assert (r["rank2"].sum(axis=-1) == n * (n + 1)).all()
    Cs = A.tocsc()
    stored = np.diff(Cs.indptr)
    empty = np.flatnonzero(stored == 0)
    assert len(empty) > 1000
    assert np.array_equal(r["rank2"][:, empty, :], np.broadcast_to((sizes * (n + 1))[:, None, :], (B, len(empty), K)))
    assert not r["npos"][:, empty, :].any() and not r["sum"][:, empty, :].any()
    assert (r["tie"][empty] == n ** 3 - n).all()
    densest = int(np.argmax(stored))
    far = int(Cs.indices[Cs.indptr[g - 1]:Cs.indptr[g]].max())
    assert densest == 12345 and stored[densest] > 2000 and far >= 65536
    sample = np.unique(np.concatenate([[0, g - 1, densest], rng.choice(np.flatnonzero(stored > 0), 61, replace=False)]))
    Xs = np.asarray(Cs[:, sample].todense(), dtype=np.float32)
    rank2, npos, sums, tie, _ = reference_stats(Xs, L, K)
    assert np.array_equal(r["rank2"][:, sample], rank2) and np.array_equal(r["npos"][:, sample], npos)
    assert np.array_equal(r["tie"][sample], tie)
    assert np.allclose(r["sum"][:, sample], sums, rtol=RTOL, atol=0.0)


# ---- 8. errors -----------------------------------------------------------------------------------------------------------

def test_errors():
    rng = np.random.default_rng(12)
    X = sparse_matrix(rng, 40, 5)
    lab = rng.integers(0, 3, 40)
    m = ExpressionMatrix(csr_of(X))
    with pytest.raises(_lib.MiSaError) as ei:
        m.rank_sum_pass(lab, 3, which="normalized")
    assert ei.value.code == ESTATE
    with pytest.raises(_lib.MiSaError) as ei:
        metrics.rank_sum_pass(m, lab, 3, which="normalized")
    assert ei.value.code == ESTATE
    with pytest.raises(_lib.MiSaError) as ei:
        m.rank_sum_pass(lab, 2, which="counts")                     # a label >= K
    assert ei.value.code == EINVAL
    same(metrics.rank_sum_pass(m, lab, 3), metrics.rank_sum_pass(X, lab, 3), "default which before normalize")
    m.close()
    with pytest.raises(ValueError):
        m.rank_sum_pass(lab, 3, which="counts")
    with pytest.raises(ValueError):
        metrics.find_all_markers(m, lab)
    big = (1 << 20) + 1
    A = sp.csr_matrix((np.ones(3, dtype=np.float32), (np.array([0, 5, big - 1]), np.zeros(3, dtype=int))), shape=(big, 1))
    with ExpressionMatrix(A) as mb:
        with pytest.raises(_lib.MiSaError) as ei:
            mb.rank_sum_pass(np.zeros(big, dtype=np.uint16), 1, which="counts")
        assert ei.value.code == EUNSUPPORTED
