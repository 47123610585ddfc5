"""The resident expression handle (csrc/prep_kernels.hip) at the gene counts and cell depths of real matrices: every loop
below has a second trip that no narrower test makes it take.  The inputs and the conditions they meet are
tests/handle_wide_cases.py's (checked off the GPU by tests/test_handle_wide_host.py); the references are those of the
narrower tests: tests/sct_correct_reference.py (equality), tests/prep_reference.py (Z bit for bit, the Gram and projection
bounds), and the dense handle, which a sparse handle must equal with ``np.array_equal``.

    test                                    loop                                                      turns from
    test_corrected_counts_wide              chunk_compact: wavefronts 1 - 3 own entries, `o += s_w[k]`  g > 1024
                                            k_sct_csr_rows: second chunk (c0 > 0, csc_first_entry       g > 4096
                                            split, s_c[j - c0], `out` carried on)
                                            k_prep_scan_counts over the genes (the new colptr): carry   g > 1024, two: g > 2048
                                            k_sct_gene_table, k_csr_block_offsets: second workgroup     listed genes, g > 256
                                            k_csr_block_hist, k_csr_block_transpose: `e += 256`         a corrected row > 256
                                            k_prep_csr_normalize's batches of 64, cell_qc's row walk    a cell stores > 64 / 256
    test_corrected_counts_many_rows         k_prep_scan_counts over the rows: carry over two tiles      n > 2048
    test_deep_* (three kinds of matrix)     csr_row_scatter (k_prep_csr_select<ScaledCols / SctCols>,   a cell stores > 256
                                            k_sct_csr_gather): `e += 256`; count > 256 columns of Z     h > 256
    test_gram_past_one_pass                 mi_prep_gram: second pass (chunk0 > 0, k_prep_gram_reduce   chunks > 256 MiB /
                                            adds onto G); tile_of with T = 32                           (64 KiB * tiles)
    test_gram_on_an_odd_number_of_tiles     tile_of with T = 17, every block against the bound          --
    test_project_at_the_feature_cap         k_prep_project over hk = 4096 features                      --

What the guard is worth, measured with a deliberately wrong build of the library that changes values only and no address
(``mi_prep_gram`` passes 0 in place of ``c0`` to ``k_prep_gram``: the second pass multiplies the first chunk's cells again,
``c1`` still keeps every read below n): see the measurements at ``test_gram_past_one_pass``.  No wrong build is made of the
corrected-count path -- a wrong offset there would hand unwritten column indices to the transpose; that its loops turn is
what the host assertions of ``handle_wide_cases.assert_corrected_coverage`` show."""
import numpy as np
import pytest
import scipy.sparse as sp

import handle_wide_cases as hw
import prep_reference as ref
import prep_regress_cases as rc
from test_gpu_prep_sparse import assert_same_passes
from test_gpu_sct import FIT_KEYS, residual_inputs
from test_gpu_sct_correct import assert_data_slot, invariant_outputs
from scrna_seq_qannealing_clustering_amd import preprocess
from scrna_seq_qannealing_clustering_amd.preprocess import ExpressionMatrix

pytestmark = pytest.mark.gpu

C = preprocess.GRAM_CHUNK


# ---- A. corrected counts past a wavefront's quarter, past a chunk, past two tiles of rows --------------------------------------

def check_corrected(n, g):
    """the sparse result against the restatement and, on every pass that reads its structure, against the dense handle's"""
    X, genes, par, lu, lu_ref, want, near = hw.corrected_case(n, g)
    assert not near.any()                                        # no entry is left out of the comparison
    labels = np.arange(n) % 3
    pick = genes[:5]
    with ExpressionMatrix(sp.csr_matrix(X)) as s, ExpressionMatrix(X) as d:
        with s.sct_correct(genes, *par, lu, lu_ref) as out, d.sct_correct(genes, *par, lu, lu_ref) as dense:
            assert out.sparse and not dense.sparse and (out.n, out.g) == (n, g) == (dense.n, dense.g)
            counts, data, nnz = out.fetch_counts(), out.fetch_normalized(), out.nnz
            dcounts, ddata = dense.fetch_counts(), dense.fetch_normalized()
            got, dgot = invariant_outputs(out, pick, labels, 3), invariant_outputs(dense, pick, labels, 3)
    # the structure: built in order, nothing stored that is zero
    assert counts.indptr[0] == 0 and counts.indptr[-1] == counts.nnz == nnz == int((want != 0).sum())
    assert np.array_equal(np.diff(counts.indptr), (want != 0).sum(axis=1))
    rows = np.repeat(np.arange(n), np.diff(counts.indptr))
    inside = rows[1:] == rows[:-1]
    assert (np.diff(counts.indices.astype(np.int64))[inside] > 0).all()          # columns strictly ascending in every row
    assert counts.indices.min() >= 0 and counts.indices.max() < g
    assert (counts.data != 0).all() and (data.data != 0).all()
    assert np.array_equal(counts.indptr, data.indptr) and np.array_equal(counts.indices, data.indices)
    # the values: the restatement's, and the dense handle's bits
    counts, data = counts.toarray(), data.toarray()
    assert counts.dtype == np.float32 and np.array_equal(counts, want.astype(np.float32)) and not np.signbit(counts).any()
    assert_data_slot(data, want)
    assert np.array_equal(counts, dcounts) and np.array_equal(data, ddata)
    # the transpose and the position map, read back through the output handle
    assert np.array_equal(got["nnz_counts"], (want != 0).sum(axis=0))
    assert np.array_equal(got["n_feature"], (want != 0).sum(axis=1))
    for key, first in dgot.items():
        assert got[key].dtype == first.dtype and np.array_equal(got[key], first, equal_nan=True), key
    return X, genes, want


@pytest.mark.parametrize("n,g", hw.CORRECTED_SHAPES)
def test_corrected_counts_wide(n, g):
    X, genes, _, _, _, want, _ = hw.corrected_case(n, g)
    hw.assert_corrected_coverage(X, genes, want)                 # (on the host: the shape does turn the loops)
    check_corrected(n, g)


@pytest.mark.parametrize("n,g", hw.ROW_SHAPES)
def test_corrected_counts_many_rows(n, g):
    assert n > 2048
    check_corrected(n, g)


# ---- B. deep cells on the sparse handle ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=hw.DEEP_KINDS)
def deep(request):
    X, A = hw.deep_case(request.param)
    hw.assert_deep(request.param, X, A)
    d, s = ExpressionMatrix(X).normalize(), ExpressionMatrix(A).normalize()
    assert s.sparse and not d.sparse
    yield request.param, X, A, d, s
    d.close()
    s.close()


def sct_parameters():
    _, lu, b0, b1, alpha = residual_inputs(hw.DEEP_N, hw.DEEP_G)
    return lu, b0, b1, alpha


def test_deep_passes(deep):
    _, X, A, _, _ = deep
    assert_same_passes(X, A)


@pytest.mark.parametrize("h", [257, 2000, preprocess.MAX_FEATURES])
def test_deep_select_gram_project(deep, h):
    _, X, A, d, s = deep
    rng = np.random.default_rng(h)
    genes = rng.permutation(hw.DEEP_G)[:h]
    if hw.DEEP_ZERO_GENE not in genes:
        genes[h // 2] = hw.DEEP_ZERO_GENE                        # an all-zero gene among them
    assert np.any(np.diff(genes) < 0) and len(set(genes.tolist())) == h
    Y = d.fetch_normalized()
    assert np.array_equal(s.fetch_normalized().toarray(), Y)
    mean, var, _ = d.gene_stats("normalized")
    mu, sigma = mean[genes], np.sqrt(var[genes])
    sigma[h // 3] = 0.0                                          # a gene the caller declares flat
    for clip in (10.0, 0.75):
        Zd, Zs = d.select(genes, mu, sigma, clip).fetch_scaled(), s.select(genes, mu, sigma, clip).fetch_scaled()
        assert Zs.shape == (hw.DEEP_N, h) and Zs.dtype == np.float32
        assert np.array_equal(Zs, Zd) and np.array_equal(Zs, ref.scaled(Y, genes, mu, sigma, clip))
        assert not Zs[:, h // 3].any() and Zs.any() and (Zs[:, genes == hw.DEEP_ZERO_GENE] == 0).all()
    assert (Zs == np.float32(0.75)).any()                        # the clip bites
    if h == 2000:
        V = rng.normal(size=(h, 7)).astype(np.float32)
        G = s.gram()
        assert np.array_equal(G, d.gram()) and G.any()
        assert np.array_equal(s.project(V), d.project(V))


def test_deep_pearson_residuals(deep):
    _, X, A, d, s = deep
    h = 2000
    lu, b0, b1, alpha = sct_parameters()
    rng = np.random.default_rng(h + 1)
    genes = rng.permutation(hw.DEEP_G)[:h]
    par = (b0[genes], b1[genes], alpha[genes])
    Q = preprocess.design_basis(rc.covariates(rng, X, 2))[0]
    out = []
    for m in (d, s):
        r = {"Z1": m.select_pearson(genes, *par, lu, center=False).fetch_scaled()}
        m.select_pearson(genes, *par, lu, Q=Q)
        r.update({"Z": m.fetch_scaled(), "coef_q": m.coef_q, "resid_mean": m.resid_mean, "resid_var": m.resid_var,
                  "flat": m.flat})
        out.append(r)
    for key, want in out[0].items():
        assert out[1][key].dtype == want.dtype and np.array_equal(out[1][key], want, equal_nan=True), key
    assert out[0]["Z1"].shape == (hw.DEEP_N, h) and out[0]["Z1"].any() and out[0]["Z"].any()


def test_deep_nb_fit_and_residual_moments(deep):
    kind, X, A, d, s = deep
    lu, b0, b1, alpha = sct_parameters()
    rng = np.random.default_rng(7)
    cells = rng.permutation(np.setdiff1d(np.arange(hw.DEEP_N), [3]))[:64]        # (row 3 is the emptied one of one kind)
    genes = rng.permutation(hw.DEEP_G)[:300]
    assert np.any(np.diff(cells) < 0) and np.any(np.diff(genes) < 0)
    fd, fs = d.nb_fit(cells, genes, lu[cells]), s.nb_fit(cells, genes, lu[cells])
    for key in FIT_KEYS:
        assert fs[key].dtype == fd[key].dtype and np.array_equal(fs[key], fd[key], equal_nan=True), key
    assert np.isfinite(fd.b1).any()
    par = (b0[genes], b1[genes], alpha[genes])
    md, ms = d.sct_residual_moments(genes, *par, lu), s.sct_residual_moments(genes, *par, lu)
    assert np.array_equal(ms[0], md[0]) and np.array_equal(ms[1], md[1]) and (md[1] > 0).any()


# ---- C. Gram past one pass of the workspace; project at the feature cap ------------------------------------------------------------

@pytest.fixture(scope="module")
def capped():
    """h = 4096 features (T = 32, 528 tiles: 7 chunks in flight) of 7 * 512 + 1 cells, the last of them heavy"""
    X, genes = hw.gram_counts()
    m = ExpressionMatrix(X).normalize()
    preprocess._select_scaled(m, genes, 10.0)
    yield m, m.fetch_scaled(), genes
    m.close()


def test_gram_past_one_pass(capped):
    """eight chunks: a pass of seven, then a pass of one chunk that holds one cell.

    MEASURED on an MI355X with the wrong build described at the top of this file (the second pass reads chunk 0): this
    test fails with max |G - G64| / bound = 3.2e4 (0.16 on the right build) and the other 32 tests of this file pass; all
    364 tests of tests/test_gpu_prep.py, test_gpu_prep_sparse.py, test_gpu_prep_regress.py, test_gpu_sct.py and
    test_gpu_sct_correct.py pass under it, as they pass on the right build -- none of them has a second pass."""
    m, Z, genes = capped
    n, h = Z.shape
    batch, chunks = hw.gram_batch(h), hw.gram_chunks(n)
    assert (n, h) == (hw.GRAM_N, hw.GRAM_H) and -(-h // hw.TILE) == 32
    assert batch < chunks                                        # the second pass runs
    heavy = np.isin(genes, np.arange(h)[hw.GRAM_HEAVY])
    assert (Z[-1, heavy] == 10.0).all() and heavy.sum() == h // 4               # the last cell is heavy: at the clip
    G = m.gram()
    again = m.gram()
    Z64 = Z.astype(np.float64)
    G64 = Z64.T @ Z64
    bound = ref.gram_bound(G64, C)
    hw.assert_gram_bound_separates(Z, G64, bound)                # (on the host: the bound tells the mistakes apart)
    assert G.shape == (h, h) and G.dtype == np.float64
    err = np.abs(G - G64)
    print("gram %d x %d: max |G - G64| / bound = %.3g" % (n, h, (err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound)
    assert np.array_equal(G, G.T)
    assert np.array_equal(G, again)


@pytest.mark.parametrize("p", [1, 128])
def test_project_at_the_feature_cap(capped, p):
    m, Z, _ = capped
    n, h = Z.shape
    V = np.random.default_rng(p).normal(size=(h, p)).astype(np.float32)
    out = m.project(V)
    assert out.shape == (n, p) and out.dtype == np.float32
    want = Z.astype(np.float64) @ V.astype(np.float64)
    assert np.abs(want).max() > 1.0
    assert np.all(np.abs(out - want) <= ref.project_bound(Z, V))
    assert np.array_equal(out, m.project(V))
    # an asymmetric operand: e_c picks column c of Z exactly, over the whole width (c * 31 mod h: up to column 3937)
    E = np.zeros((h, p), dtype=np.float32)
    pick = np.arange(p) * 31 % h
    E[pick, np.arange(p)] = 1.0
    assert np.array_equal(m.project(E), Z[:, pick])


def test_gram_on_an_odd_number_of_tiles():
    """h = 2049: ldz = 2176, T = 17, 153 tiles in one pass; every block of G differs from zero and obeys the bound, the last
    block row and column are one feature wide"""
    n, h = C + 1, 2049
    assert hw.gram_batch(h) >= hw.gram_chunks(n)
    rng = np.random.default_rng(17)
    with ExpressionMatrix(ref.sparse_counts(rng, n, h, rate=0.5)).normalize() as m:
        preprocess._select_scaled(m, rng.permutation(h), 10.0)
        Z = m.fetch_scaled().astype(np.float64)
        G = m.gram()
    G64 = Z.T @ Z
    bound = ref.gram_bound(G64, C)
    T = -(-h // hw.TILE)
    assert T == 17
    for a in range(T):
        for b in range(T):
            blk = (slice(hw.TILE * a, hw.TILE * a + hw.TILE), slice(hw.TILE * b, hw.TILE * b + hw.TILE))
            assert np.abs(G64[blk]).max() > 1.0, (a, b)
            assert np.all(np.abs(G[blk] - G64[blk]) <= bound[blk]), (a, b)
    assert np.array_equal(G, G.T) and G.shape == (h, h)
