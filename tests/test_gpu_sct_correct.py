"""SCTransform's corrected counts and ``data`` slot on the device (``mi_prep_sct_correct``, ``mi_prep_fetch_counts``,
``mi_prep_fetch_csr``; ``ExpressionMatrix.sct_correct``, ``sctransform(return_corrected=True)``) against the numpy fp64
restatement of tests/sct_correct_reference.py.

Corrected counts are integers: device and restatement are compared for EQUALITY.  An entry could differ only where
``mu_r + r s_r`` lies within 1e-9 of a half-integer; every test asserts that its inputs have no such entry, so none is left
out (tests/test_sct_correct_host.py prints the nearest: 4.7e-6 over these shapes).  The data slot is ``float32(log1p(c))``
within one ulp of float32, exact where c is 0.  Sparse against dense and run against run: ``np.array_equal`` on everything."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import prep_regress_cases as rc
import sct_cases as sc
import sct_correct_reference as cr
from scrna_seq_qannealing_clustering_amd import _lib, metrics, preprocess
from scrna_seq_qannealing_clustering_amd.preprocess import ExpressionMatrix

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -5
SHAPES = [(n, 65) for n in (2, 255, 256, 257, 1027)] + [(257, g) for g in (1, 63, 64, 65, 150)]


def assert_data_slot(data, c):
    """float32(log1p(c)) within 1 ulp of float32, exact where c is 0"""
    want = cr.data_slot(c)
    assert data.dtype == np.float32 and data.shape == c.shape
    assert np.all(np.abs(data.astype(np.float64) - want) <= np.spacing(want).astype(np.float64))
    assert np.array_equal(data[c == 0], np.zeros(int((c == 0).sum()), dtype=np.float32))
    assert not np.signbit(data).any()


@pytest.mark.parametrize("kind", ["dense", "csr"])
@pytest.mark.parametrize("n,g", SHAPES)
def test_values_equal_the_restatement(n, g, kind):
    X, lu, b0, b1, alpha, lu_ref = cr.inputs(n, g)
    genes = cr.listed_genes(g)
    assert len(genes) == (g if g == 1 else (2 * g + 2) // 3) and (g < 3 or not np.array_equal(genes, np.sort(genes)))
    want, near = cr.corrected(X, genes, b0[genes], b1[genes], alpha[genes], lu, lu_ref)
    assert not near.any()                                        # no entry is left out of the comparison
    with ExpressionMatrix(sp.csr_matrix(X) if kind == "csr" else X) as src:
        with src.sct_correct(genes, b0[genes], b1[genes], alpha[genes], lu, lu_ref) as out:
            assert out.sparse == (kind == "csr") and (out.n, out.g) == (n, g) and out.normalized
            counts, data = out.fetch_counts(), out.fetch_normalized()
            nnz = out.nnz
        assert src.timing["sct_correct_ms"] >= 0.0
    if kind == "csr":
        assert sp.issparse(counts) and counts.shape == (n, g) and counts.dtype == np.float32 and counts.nnz == nnz
        assert nnz == int((want != 0).sum()) and (counts.data != 0).all()
        assert np.array_equal(counts.indptr, data.indptr) and np.array_equal(counts.indices, data.indices)
        counts, data = counts.toarray(), data.toarray()
    assert counts.dtype == np.float32 and counts.shape == (n, g)
    assert np.array_equal(counts, want.astype(np.float32)) and not np.signbit(counts).any()
    off = np.setdiff1d(np.arange(g), genes)
    assert not counts[:, off].any() and not data[:, off].any()
    assert_data_slot(data, want)
    if n >= 255 and g >= 63:                                     # the structure is built, not copied: both directions occur
        Xg, cg = X[:, genes], want[:, genes]
        assert ((Xg == 0) & (cg != 0)).any() and ((Xg != 0) & (cg == 0)).any()


@pytest.mark.parametrize("kind", ["dense", "csr"])
@pytest.mark.parametrize("n,g", [(257, 65), (1027, 150), (2, 1)])
def test_identity_at_the_reference_depth(n, g, kind):
    """every cell at the reference depth: mu == mu_r, so integer counts come back as they are, whatever the parameters --
    a check of the gene / cell indexing that does not go through the restatement"""
    X, _, b0, b1, alpha, _ = cr.inputs(n, g)
    genes = cr.listed_genes(g, seed=1)
    lu = np.full(n, 3.21)
    with ExpressionMatrix(sp.csr_matrix(X) if kind == "csr" else X) as src, \
            src.sct_correct(genes, b0[genes], b1[genes], alpha[genes], lu, 3.21) as out:
        counts = out.fetch_counts()
    counts = counts.toarray() if kind == "csr" else counts
    want = np.zeros_like(X)
    want[:, genes] = X[:, genes]
    assert np.array_equal(counts, want) and want.any()


# ---- sparse equals dense, run equals run --------------------------------------------------------------------------------------

def invariant_outputs(m, genes, labels, K):
    """every pass that reads another part of the handle's invariant"""
    out = {}
    for which in ("counts", "normalized"):
        out["mean_" + which], out["var_" + which], out["nnz_" + which] = m.gene_stats(which)      # the transpose
    out["n_count"], out["n_feature"], _ = m.cell_qc()                                            # the CSR
    out["log1p"] = m.gene_log1p_sum()
    for gather in ("inplace", "permute"):                                                        # the position map
        r = m.rank_sum_pass(labels, K, which="normalized", gather=gather)
        out.update({"%s_%s" % (key, gather): r[key] for key in ("rank2", "npos", "sum", "tie")})
    mean, var, _ = m.gene_stats("normalized")
    m.select(genes, mean[genes], np.sqrt(var[genes]))
    out["Z"], out["gram"] = m.fetch_scaled(), m.gram()
    return out


@pytest.mark.parametrize("n,g", [(257, 150), (1027, 150), (255, 1)])
def test_sparse_equals_dense_and_run_equals_run(n, g):
    X, lu, b0, b1, alpha, _ = cr.inputs(n, g, seed=9)
    X, lu, b0 = X.copy(), lu.copy(), b0.copy()
    lu[3] = 4.5                                                  # the emptied cell is the deepest: its corrected row is all zero
    genes = cr.listed_genes(g, seed=2)
    dead = int(genes[0]) if g > 1 else None                      # a listed gene without counts and with a tiny mean
    if dead is not None:
        X[:, dead] = 0.0
        b0[dead] = -25.0
    X, A = rc.csr_with_stored_zeros_and_empty_row(X, np.random.default_rng(n))
    assert (A.data == 0).any() and A.indptr[3] == A.indptr[4]
    lu_ref = cr.reference_depth(lu)
    par = (b0[genes], b1[genes], alpha[genes])
    want, near = cr.corrected(X, genes, *par, lu, lu_ref)
    assert not near.any() and not want[3].any() and (dead is None or not want[:, dead].any())
    labels = np.arange(n) % 3
    pick = genes[:min(len(genes), 5)] if g > 1 else genes
    results, fetched = [], []
    with ExpressionMatrix(X) as d, ExpressionMatrix(A) as s:
        for src in (d, s, d, s):
            with src.sct_correct(genes, *par, lu, lu_ref) as out:
                assert out.sparse == src.sparse
                counts, data = out.fetch_counts(), out.fetch_normalized()
                if out.sparse:
                    assert counts.indptr[0] == 0 and counts.indptr[-1] == counts.nnz == out.nnz
                    assert counts.has_sorted_indices and (counts.data != 0).all() and (data.data != 0).all()
                    for i in range(n):                           # columns strictly ascending inside every row
                        assert (np.diff(counts.indices[counts.indptr[i]:counts.indptr[i + 1]]) > 0).all()
                    assert np.array_equal(counts.indptr, data.indptr) and np.array_equal(counts.indices, data.indices)
                    counts, data = counts.toarray(), data.toarray()
                fetched.append((counts, data))
                results.append(invariant_outputs(out, pick, labels, 3))
    assert np.array_equal(fetched[0][0], want.astype(np.float32))
    assert_data_slot(fetched[0][1], want)
    for counts, data in fetched[1:]:
        assert np.array_equal(counts, fetched[0][0]) and np.array_equal(data, fetched[0][1])
    for other in results[1:]:
        for key, first in results[0].items():
            assert other[key].dtype == first.dtype and np.array_equal(other[key], first, equal_nan=True), key
    assert np.array_equal(results[0]["nnz_counts"], (want != 0).sum(axis=0))
    assert np.array_equal(results[0]["n_feature"], (want != 0).sum(axis=1)) and results[0]["n_feature"][3] == 0


# ---- the source is untouched ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["dense", "csr"])
def test_source_is_untouched_and_may_be_closed_first(kind):
    X, lu, b0, b1, alpha, lu_ref = cr.inputs(257, 65)
    genes = cr.listed_genes(65)
    want, _ = cr.corrected(X, genes, b0[genes], b1[genes], alpha[genes], lu, lu_ref)
    src = ExpressionMatrix(sp.csr_matrix(X) if kind == "csr" else X)
    src.normalize()
    dense = (lambda M: M.toarray() if kind == "csr" else M)
    bytes0, norm0, stats0 = src.device_bytes(), dense(src.fetch_normalized()), src.gene_stats("counts")
    out = src.sct_correct(genes, b0[genes], b1[genes], alpha[genes], lu, lu_ref)
    src._stats.clear()                                           # (gene_stats caches on the Python side: ask the device again)
    assert src.device_bytes() == bytes0 and np.array_equal(dense(src.fetch_normalized()), norm0)
    for a, b in zip(src.gene_stats("counts"), stats0):
        assert np.array_equal(a, b)
    assert np.array_equal(dense(src.fetch_counts()), X)
    src.close()
    assert np.array_equal(dense(out.fetch_counts()), want.astype(np.float32))
    assert np.array_equal(out.gene_stats("counts")[2], (want != 0).sum(axis=0))
    assert out.device_bytes() > 0
    out.close()
    with pytest.raises(ValueError):
        out.fetch_counts()


# ---- errors ---------------------------------------------------------------------------------------------------------------------

def code_of(fn, *args, **kw):
    with pytest.raises(_lib.MiSaError) as ei:
        fn(*args, **kw)
    return ei.value.code


@pytest.mark.parametrize("kind", ["dense", "csr"])
def test_errors(kind):
    X, lu, b0, b1, alpha, lu_ref = cr.inputs(12, 6)
    genes, one = np.arange(3, dtype=np.int32), np.ones(3)
    p3 = (b0[:3].copy(), b1[:3].copy(), alpha[:3].copy())
    f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    ptr = lambda a, t: a.ctypes.data_as(t)
    with ExpressionMatrix(sp.csr_matrix(X) if kind == "csr" else X) as m:
        lib, h = m._lib, m._handle()
        bytes0 = m.device_bytes()
        out = C.c_void_p(1)

        def raw(h_=h, genes_=genes, gp=3, b0_=p3[0], b1_=p3[1], al=p3[2], lu_=lu, ref=lu_ref, out_=out):
            out.value = 1
            return lib.mi_prep_sct_correct(h_, None if genes_ is None else ptr(genes_, i32p), gp,
                                           *[None if a is None else ptr(np.ascontiguousarray(a, dtype=np.float64), f64p)
                                             for a in (b0_, b1_, al, lu_)], ref, None if out_ is None else C.byref(out_), None)

        # NULL arguments
        assert raw(h_=None) == EINVAL and not out.value
        for name in ("genes_", "b0_", "b1_", "al", "lu_"):
            assert raw(**{name: None}) == EINVAL and not out.value
        assert raw(out_=None) == EINVAL
        # gp outside [1, g]
        assert raw(gp=0) == EINVAL and raw(gp=7) == EINVAL and not out.value
        # a gene out of range or repeated
        assert raw(genes_=np.array([0, 1, 6], dtype=np.int32)) == EINVAL and raw(genes_=np.array([0, -1, 2], dtype=np.int32)) == EINVAL
        assert raw(genes_=np.array([0, 1, 1], dtype=np.int32)) == EINVAL and not out.value
        # non-finite b0, b1, log_umi, log_umi_ref
        bad_lu = lu.copy()
        bad_lu[4] = np.nan
        assert raw(b0_=one * np.nan) == EINVAL and raw(b1_=one * np.inf) == EINVAL and raw(lu_=bad_lu) == EINVAL
        assert raw(ref=np.inf) == EINVAL and raw(ref=np.nan) == EINVAL and not out.value
        # alpha negative or not finite
        assert raw(al=-one) == EINVAL and raw(al=one * np.inf) == EINVAL and raw(al=one * np.nan) == EINVAL and not out.value
        # found on the device: an overflowing mean
        assert raw(b0_=np.array([p3[0][0], 800.0, p3[0][2]])) == EINVAL and not out.value
        assert b"finite" in lib.mi_last_error()
        assert code_of(m.sct_correct, genes, [p3[0][0], 800.0, p3[0][2]], p3[1], p3[2], lu, lu_ref) == EINVAL
        assert code_of(m.sct_correct, genes, p3[0], p3[1], p3[2], lu, 400.0) == EINVAL          # ... at the reference depth
        with pytest.raises(ValueError):
            m.sct_correct(genes, *p3, bad_lu, lu_ref)
        with pytest.raises(ValueError):
            m.sct_correct(genes, p3[0][:2], p3[1], p3[2], lu, lu_ref)
        assert m.device_bytes() == bytes0
        # the fetch entries
        buf = np.empty(12 * 6, dtype=np.float32)
        if kind == "csr":
            assert lib.mi_prep_fetch_counts(h, ptr(buf, C.POINTER(C.c_float))) == EUNSUPPORTED
            assert lib.mi_prep_fetch_csr(h, None, None, None) == 0
        else:
            assert lib.mi_prep_fetch_csr(h, None, None, ptr(buf, C.POINTER(C.c_float))) == EINVAL
            assert lib.mi_prep_fetch_counts(h, None) == EINVAL
        # ... and after all that the handle still works
        with m.sct_correct(genes, *p3, lu, lu_ref) as ok:
            assert ok.fetch_counts().shape == (12, 6)
    with pytest.raises(ValueError, match="closed"):
        m.sct_correct(genes, *p3, lu, lu_ref)
    with pytest.raises(ValueError, match="closed"):
        m.fetch_counts()


def test_more_than_max_nnz_corrected_entries_are_refused():
    """65536 x 32768 = 2^31 cells of an empty CSR, every one shallower than the reference depth under a large mean: every zero
    becomes a count, one entry more than MI_PREP_MAX_NNZ.  The scanned total (64-bit) finds it; nothing of that size is
    allocated."""
    n, g = 65536, 32768
    A = sp.csr_matrix((n, g), dtype=np.float32)
    with ExpressionMatrix(A) as m:
        bytes0 = m.device_bytes()
        code = code_of(m.sct_correct, np.arange(g), np.full(g, -4.0), np.full(g, 2.3), np.zeros(g), np.full(n, 3.0), 4.0)
        assert code == EUNSUPPORTED and m.device_bytes() == bytes0
        assert b"exceed" in m._lib.mi_last_error()


def test_a_result_without_entries_is_a_valid_handle():
    """a reference depth below every cell of an empty matrix leaves nothing at all"""
    n, g = 300, 70
    with ExpressionMatrix(sp.csr_matrix((n, g), dtype=np.float32)) as m:
        with m.sct_correct(np.arange(g), np.full(g, -4.0), np.full(g, 2.3), np.zeros(g), np.full(n, 3.0), 2.0) as out:
            counts = out.fetch_counts()
            assert out.nnz == 0 and counts.nnz == 0 and counts.shape == (n, g) and not counts.indptr.any()
            assert not out.gene_stats("counts")[2].any() and not out.cell_qc()[1].any()
            assert out.fetch_normalized().nnz == 0


# ---- the driver -----------------------------------------------------------------------------------------------------------------

TOP = 20


def driver_runs():
    X, groups, marker = sc.planted_counts()
    plain = preprocess.sctransform(X, variable_features_n=200, npcs=10)
    dense = preprocess.sctransform(X, variable_features_n=200, npcs=10, return_corrected=True)
    csr = preprocess.sctransform(sp.csr_matrix(X), variable_features_n=200, npcs=10, return_corrected=True)
    return X, groups, marker, plain, dense, csr


def assert_same(a, b, path=""):
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for key in a:
            assert_same(a[key], b[key], path + "." + str(key))
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), path


def test_driver_returns_the_corrected_handle():
    """MEASURED on the numpy restatement of the whole chain (tests/sct_reference.py's driver, then
    tests/sct_correct_reference.py at log10 of the median total; avg_log2FC of log1p(c) and Seurat's filter evaluated in
    numpy): for each of the three planted groups the 40 genes with the largest avg_log2FC are exactly its 40 planted
    markers (120, 132 and 123 genes pass the filter); the nearest value to a half-integer is 2.0e-6.  The assertion
    demands the top TOP = 20 per group, half of what the restatement delivers."""
    X, groups, marker, plain, dense, csr = driver_runs()
    try:
        cd, cs = dense["corrected"], csr["corrected"]
        assert isinstance(cd, ExpressionMatrix) and not cd.sparse and cs.sparse and cd.normalized and cs.normalized
        assert (cd.n, cd.g) == X.shape == (cs.n, cs.g)
        assert "corrected" not in plain and "median_umi" not in plain and "sct_correct_ms" not in plain.timing
        assert dense.median_umi == csr.median_umi == float(np.median(X.astype(np.float64).sum(axis=1)))
        assert dense.timing["sct_correct_ms"] >= 0.0 and csr.timing["sct_correct_ms"] >= 0.0
        # every other field is that of the call without the flag
        for r in (dense, csr):
            assert set(r) - {"corrected", "median_umi"} == set(plain)
            assert set(r.timing) - {"sct_correct_ms", "create_s"} == set(plain.timing)
            for key in plain:
                if key != "timing":
                    assert_same(r[key], plain[key], key)
        # identical bits, dense and sparse, and the restatement at the device's parameters
        counts, data = cd.fetch_counts(), cd.fetch_normalized()
        assert np.array_equal(cs.fetch_counts().toarray(), counts) and np.array_equal(cs.fetch_normalized().toarray(), data)
        a = dense.gene_attr
        passing = np.flatnonzero(a.passing)
        want, near = cr.corrected(X, passing, a.b0[passing], a.b1[passing], a.alpha[passing], dense.log_umi,
                                  np.log10(dense.median_umi))
        assert not near.any() and np.array_equal(counts, want.astype(np.float32))
        assert_data_slot(data, want)
        # markers on the resident data slot: the planted genes lead every group
        found = {}
        for name, handle in (("dense", cd), ("csr", cs)):
            res = metrics.find_all_markers(handle, groups)
            found[name] = res
            top = metrics.top_markers(res, n=TOP)
            for c in range(sc.PLANTED["groups"]):
                own = np.arange(sc.PLANTED["markers"] * c, sc.PLANTED["markers"] * (c + 1))
                assert len(top[c]) == TOP and np.isin(top[c], own).all(), (name, c, top[c])
        for key in ("U", "p_val", "avg_log2FC", "pct_1", "pct_2", "passed"):
            assert np.array_equal(found["dense"][key], found["csr"][key], equal_nan=True), key
        labels = np.stack([groups, (groups + 1) % 3])
        for gather in (None, "inplace", "permute"):
            rd, rs = cd.rank_sum_pass(labels, 3), cs.rank_sum_pass(labels, 3, gather=gather)
            for key in ("rank2", "npos", "sum", "tie"):
                assert np.array_equal(rd[key], rs[key]), key
        # the benchmark chain: cluster statistics from either kind of handle, field for field
        sd = metrics.cluster_stats(data, groups)
        ss = metrics.cluster_stats(cs.fetch_normalized(), groups)
        assert set(sd) == set(ss)
        for key in sd:
            if key != "kernel_ms":
                assert np.array_equal(np.asarray(sd[key]), np.asarray(ss[key]), equal_nan=True), key
        assert sd["average.within"] < sd["average.between"]
    finally:
        dense["corrected"].close()
        csr["corrected"].close()
