"""Inputs of the wide-handle tests (tests/test_handle_wide_host.py off the GPU, tests/test_gpu_handle_wide.py on it): the
shapes at which the loops of the resident expression handle take their second trip, and the conditions on those inputs that
the GPU tests rely on, as functions both files call -- if a generator changes, the host test says so without a GPU.

Nothing here is a reference of its own: the corrected counts are tests/sct_correct_reference.py's, the scaled matrix
tests/prep_reference.py's."""
import functools

import numpy as np

import prep_reference as ref
import prep_regress_cases as rc
import prep_sparse_cases as cases
import sct_correct_reference as cr
from scrna_seq_qannealing_clustering_amd import preprocess

CORR_CHUNK = 4096                             # kCorrChunk (csrc/prep_kernels.hip): genes of a cell in LDS at a time
CORR_QUARTER = CORR_CHUNK // 4                # the part of a chunk one of the four wavefronts compacts
TILE = 128                                    # the Gram tile (kTile)

# g: the last quarter of one column (1025, 2049, 3073), a full chunk less one / exactly / plus one (4095, 4096, 4097), a second
# chunk of one ballot (4160), three chunks (8195); n = 40 and 70: two and three row blocks of the transpose (R = 32)
CORRECTED_SHAPES = [(40, g) for g in (1023, 1025, 2049, 3073, 4095, 4096, 4097, 4160)] + [(70, 8195)]
ROW_SHAPES = [(2051, 65), (3000, 65)]         # k_prep_scan_counts over the rows: a carry over two tiles of 1024


@functools.lru_cache(maxsize=None)
def corrected_case(n, g):
    """-> X, genes (``listed_genes`` and gene g - 1), (b0, b1, alpha) of the genes, log_umi, log_umi_ref, and the
    restatement's corrected counts and near-half marks"""
    X, lu, b0, b1, alpha, lu_ref = cr.inputs(n, g)
    genes = cr.listed_genes(g)
    if g - 1 not in genes:
        genes = np.append(genes, g - 1).astype(np.int32)
    par = (b0[genes], b1[genes], alpha[genes])
    want, near = cr.corrected(X, genes, *par, lu, lu_ref)
    want.setflags(write=False)
    return X, genes, par, lu, lu_ref, want, near


def quarters(g):
    """the column ranges [lo, hi) a wavefront of ``chunk_compact`` owns, over every chunk a row of g genes reaches"""
    out = []
    for c0 in range(0, g, CORR_CHUNK):
        for lo in range(c0, min(c0 + CORR_CHUNK, g), CORR_QUARTER):
            out.append((lo, min(lo + CORR_QUARTER, c0 + CORR_CHUNK, g)))
    return out


def assert_corrected_coverage(X, genes, want):
    """every wavefront's quarter of every chunk compacts a zero that became a count and a stored count that stayed one, and
    skips an unlisted gene; some row has entries in two chunks when there are two; the gene table has a second workgroup.

    A tail quarter narrower than one ballot of 64 lanes cannot promise all three: the one-column tails (g = 1025, 2049, 3073,
    4097) are gene g - 1, which is listed by construction, and one gene over 40 cells need not hold both kinds of entry
    (at g = 3073 no zero of it becomes a count); the three columns of g = 8195's last chunk are all listed.  Of such a
    quarter it is asserted that its wavefront has an entry to emit; the wavefront's full-width turn is another shape's."""
    g = X.shape[1]
    listed = np.zeros(g, dtype=bool)
    listed[genes] = True
    assert listed.sum() > 256
    for lo, hi in quarters(g):
        x, c = X[:, lo:hi], want[:, lo:hi]
        assert not c[:, ~listed[lo:hi]].any()
        if hi - lo < 64:
            assert (hi - lo in (1, 3)) and hi == g and (c != 0).any(), (g, lo, hi)
            continue
        assert ((x == 0) & (c != 0)).any(), (g, lo, hi)
        assert ((x != 0) & (c != 0)).any(), (g, lo, hi)
        assert not listed[lo:hi].all(), (g, lo, hi)
    if g > CORR_CHUNK:
        per_chunk = np.stack([(want[:, c0:c0 + CORR_CHUNK] != 0).any(axis=1) for c0 in range(0, g, CORR_CHUNK)])
        assert (per_chunk.sum(axis=0) >= 2).any()


# ---- deep cells ---------------------------------------------------------------------------------------------------------------

DEEP_N, DEEP_G = 70, 4100
DEEP_KINDS = ("rate0.3", "wide", "stored_zeros")
DEEP_ZERO_GENE = 11


@functools.lru_cache(maxsize=None)
def deep_case(kind):
    """-> (X dense, A csr of it): 70 cells of about 1060 stored entries each, gene 11 all zero.  ``stored_zeros``: the
    rate-0.3 counts with row 3 emptied and a tenth of the zeros stored"""
    rng = np.random.default_rng(1000 * DEEP_N + DEEP_G)
    X = cases.GENERATORS["wide" if kind == "wide" else "rate0.3"](rng, DEEP_N, DEEP_G)
    X[:, DEEP_ZERO_GENE] = 0.0
    if kind == "stored_zeros":
        X, A = rc.csr_with_stored_zeros_and_empty_row(X, rng)
    else:
        import scipy.sparse as sp
        A = sp.csr_matrix(X)
    X.setflags(write=False)
    return X, A


def assert_deep(kind, X, A):
    """every cell stores more than 256 entries (the emptied row of ``stored_zeros`` aside): ``csr_row_scatter`` and the row
    walks of the sparse kernels step at least twice, most of them five times"""
    stored = np.diff(A.indptr)
    keep = np.ones(len(stored), dtype=bool)
    if kind == "stored_zeros":
        assert stored[3] == 0 and (A.data == 0).any()
        keep[3] = False
    assert (stored[keep] > 256).all() and stored.max() > 1024
    assert not X[:, DEEP_ZERO_GENE].any()


# ---- Gram ----------------------------------------------------------------------------------------------------------------------

def gram_batch(h):
    """chunks of GRAM_CHUNK cells whose tiles one pass of ``mi_prep_gram`` keeps in flight (include/mi_prep.h)"""
    T = (h + TILE - 1) // TILE
    return max(1, preprocess.GRAM_WORKSPACE // (TILE * TILE * 4 * (T * (T + 1) // 2)))


GRAM_H = preprocess.MAX_FEATURES                                 # T = 32, 528 tiles: 7 chunks in flight
GRAM_N = gram_batch(GRAM_H) * preprocess.GRAM_CHUNK + 1          # a pass of `batch` chunks, then one chunk of one cell
GRAM_HEAVY = slice(0, None, 4)                                   # the genes only the last cell expresses


def gram_chunks(n):
    return (n + preprocess.GRAM_CHUNK - 1) // preprocess.GRAM_CHUNK


@functools.lru_cache(maxsize=None)
def gram_counts(n=GRAM_N, h=GRAM_H, seed=3):
    """the recipe of tests/test_gpu_prep.py's ``scaled_handle`` with a heavy last cell: every fourth gene has its only
    counts there, so its scaled value is sqrt(n) before the clip and 10 after it.  -> (X, the genes' order)"""
    rng = np.random.default_rng(seed)
    X = ref.sparse_counts(rng, n, h, rate=0.5)
    X[:-1, GRAM_HEAVY] = 0.0
    X[-1, GRAM_HEAVY] = rng.integers(1, 21, len(range(h)[GRAM_HEAVY]))
    X.setflags(write=False)
    return X, rng.permutation(h)


def assert_gram_bound_separates(Z, G64, bound):
    """the two mistakes a second pass can make are outside the bound: a last pass that never ran (or ran on the first
    chunk again and was dropped), and a first chunk counted twice"""
    Z64 = np.asarray(Z, dtype=np.float64)
    n, C = Z64.shape[0], preprocess.GRAM_CHUNK
    batch, chunks = gram_batch(Z64.shape[1]), gram_chunks(n)
    assert 1 <= batch < chunks
    tail = Z64[batch * C:]
    without_last_pass = G64 - tail.T @ tail
    assert (np.abs(without_last_pass - G64) > bound).any()
    first = Z64[:C]
    first_twice = G64 + first.T @ first
    assert (np.abs(first_twice - G64) > bound).any()
    # ... and the mistake of reading chunk 0 in place of the last pass's chunks, which is both at once
    assert (np.abs(first_twice - tail.T @ tail - G64) > bound).any()
