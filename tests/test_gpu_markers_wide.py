"""The rank-sum marker pass (csrc/markers_kernels.hip) with more genes than workgroups.  ``k_markers_rank`` strides over the
genes with a grid of 8 workgroups per compute unit, capped at g (csrc/mi_markers_plan.h); the edge tests have g <= 200, so
each workgroup ranks exactly one gene there, and the one wide matrix (``test_beyond_the_dense_limits``: a CSR handle, about
three entries per gene) is compared on a sample of 64 genes and on its empty ones.  Here g = 2 * grid + 65: every workgroup
ranks two genes, the first 65 rank three, and every gene is compared.  The references are the narrower tests': ``markers_reference.reference_stats`` (integers with ``np.array_equal``,
plain sums bit for bit, expm1 sums within the project's 1e-9) and the dense entry point, which a handle must equal.

    test                                      loop                                                        turns from
    test_three_genes_per_workgroup            k_markers_rank's gene loop: the resets of s_tie, s_cnt,     g > 8 * CUs
                                              acc and negc between genes; with force_global the reuse of
                                              a workgroup's HBM slab
    test_three_genes_per_workgroup_on_handles the same on a CSR and a dense handle, both gathers           g > 8 * CUs
    test_slab_and_lds_genes_in_one_workgroup  an LDS gene after a slab gene and before one; the            g > 8 * CUs, a gene
                                              labelling chunk loop turns twice per gene (B = 17)           above the LDS cap

The special columns of tests/test_gpu_markers.py stand where one workgroup meets them in an awkward order (j, j + grid,
j + 2 grid): a gene that is one tie group, then an all-zero gene, then an all-distinct one (a stale tie sum, count or
midrank shows as a wrong ``tie`` or ``rank2``); a gene with negatives before genes without (a stale ``negc`` shows as a
wrong ``npos``).

What the guard is worth, measured with a deliberately wrong build of the library that changes values only and no address
(``rank_gene`` clears ``*s_tie`` for a workgroup's first gene only): see the measurements at
``test_three_genes_per_workgroup``."""
import numpy as np
import pytest

from markers_reference import reference_stats, sparse_matrix
from test_gpu_markers import check_integers, special_columns
from test_gpu_markers_sparse import check_handle, csr_of, same
from scrna_seq_qannealing_clustering_amd import _lib, metrics
from scrna_seq_qannealing_clustering_amd.preprocess import ExpressionMatrix

pytestmark = pytest.mark.gpu

RTOL = 1e-9                                   # the project's fp64 tolerance (tests/test_gpu_markers.py)
CAP = metrics.MARKERS_LDS_MAX_NONZEROS
CHUNK = metrics.MARKERS_LABELLING_CHUNK
N, B, K = 70, 2, 3


def grid_and_genes():
    grid = 8 * _lib.device_info(0)["compute_units"]
    g = 2 * grid + 65
    assert g > 2 * grid
    return grid, g


# residue -> the special columns workgroup `residue` ranks as its first, second and third gene
PLACED = {5: ("one_tie_group", "all_zero", "all_distinct"),
          40: ("normal", "no_zeros", "counts_0_3"),
          64: ("both_zeros", "all_zero", "normal")}


_cache = {}


def wide_case():
    """-> grid, X (70 x g, the special columns placed), L (2 x 70), the reference's results without and with plain sums"""
    if not _cache:
        grid, g = grid_and_genes()
        rng = np.random.default_rng(21)
        X = sparse_matrix(rng, N, g)
        names, S = special_columns(rng)                          # (300 cells: the first 70 keep what makes each column special)
        S = S[:N]
        for j, trio in PLACED.items():
            for k, name in enumerate(trio):
                assert j + k * grid < g
                X[:, j + k * grid] = S[:, names.index(name)]
        tie_group, zero, distinct, normal = (X[:, j] for j in (5, 5 + grid, 5 + 2 * grid, 40))
        assert len(set(tie_group.tolist())) == 1 and not zero.any() and len(set(distinct.tolist())) == N
        assert (normal < 0).any() and (X[:, 40 + grid] > 0).all() and (X[:, g - 1] < 0).any()
        z = X[:, 64]
        assert np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all() and (z < 0).any()
        L = rng.integers(0, K, (B, N))
        X.setflags(write=False)
        _cache["case"] = (grid, X, L, reference_stats(X, L, K), reference_stats(X, L, K, plain=True))
    return _cache["case"]


def test_three_genes_per_workgroup():
    """MEASURED on an MI355X with the wrong build described at the top of this file: all three tests of this file fail
    (``tie`` of a gene that is not its workgroup's first carries the genes before it: 990 where the all-distinct last gene
    has 0).  Of the 54 tests of tests/test_gpu_markers.py and tests/test_gpu_markers_sparse.py 53 pass under it; the one
    that fails is ``test_beyond_the_dense_limits``, whose 65 536 genes on a CSR handle do give a workgroup many genes, the
    empty ones with a known tie term.  So this one reset was guarded before, on the CSR source in the LDS form; the dense
    source, the slab's reuse, slab next to LDS genes, ``negc``, ``acc`` and the midranks of non-empty genes were not."""
    grid, X, L, want, want_plain = wide_case()
    g = X.shape[1]
    r = check_integers(X, L, K)                                  # the LDS form and the forced HBM form: a slab used three times
    assert r["tie"][5] == N ** 3 - N == r["tie"][5 + grid] and r["tie"][5 + 2 * grid] == 0
    assert (r["rank2"].sum(axis=2) == N * (N + 1)).all()         # whatever the labelling
    assert np.array_equal(r["npos"].sum(axis=2), np.broadcast_to((X > 0).sum(axis=0), (B, g)))
    assert np.allclose(r["sum"], want[2], rtol=RTOL, atol=0.0)
    for force in (False, True):
        p = metrics.rank_sum_pass(X, L, K, plain=True, force_global=force)
        assert np.array_equal(p["sum"], want_plain[2])           # the same additions in the same order
        for key in ("rank2", "npos", "tie"):
            assert np.array_equal(p[key], r[key]), key


def test_three_genes_per_workgroup_on_handles():
    """the same genes on the resident handle, CSR and dense (no negative values there: the matrix is |X|), in the LDS and
    the HBM form and with both ways of reading a sparse handle's values, against the dense entry point"""
    grid, X, L, _, _ = wide_case()
    Xp = np.abs(X)
    assert not np.signbit(Xp).any()
    for plain in (False, True):
        want = reference_stats(Xp, L, K, plain=plain)
        entry = metrics.rank_sum_pass(Xp, L, K, plain=plain)
        with ExpressionMatrix(csr_of(Xp)) as m:
            assert m.sparse
            r = check_handle(m, Xp, L, K, want, entry, plain=plain)
        with ExpressionMatrix(Xp) as m:
            same(r, check_handle(m, Xp, L, K, want, entry, plain=plain), "dense handle")
        if plain:
            assert np.array_equal(r["sum"], want[2])
        else:
            assert np.allclose(r["sum"], want[2], rtol=RTOL, atol=0.0)


def test_slab_and_lds_genes_in_one_workgroup():
    """n = CAP + 16 cells, B = CHUNK + 1 labellings; every gene stores about six entries and is ranked in LDS, except three
    of CAP + 1 non-zeros at j, j + grid and j + 2 grid of three different residues, which go through their workgroup's HBM
    slab: one workgroup ranks slab, LDS, LDS, another LDS, slab, LDS, a third LDS, LDS, slab"""
    grid, g = grid_and_genes()
    n, nb, k = CAP + 16, CHUNK + 1, 4
    heavy = (7, grid + 21, 2 * grid + 50)
    assert len({j % grid for j in heavy}) == 3 and [j // grid for j in heavy] == [0, 1, 2] and max(heavy) < g
    assert grid * 2 * (CAP + 1) * 12 <= 1 << 30                  # the slab budget leaves the grid at 8 per compute unit
    rng = np.random.default_rng(22)
    X = np.zeros((n, g), dtype=np.float32)
    X[rng.integers(0, n, 6 * g), np.repeat(np.arange(g), 6)] = np.round(rng.uniform(0.1, 3.0, 6 * g), 1)
    for j in heavy:
        X[:, j] = 0.0
        X[rng.permutation(n)[:CAP + 1], j] = np.round(rng.uniform(0.1, 3.0, CAP + 1), 2)      # (two decimals: ties)
    stored = (X != 0).sum(axis=0)
    assert (stored[list(heavy)] == CAP + 1).all() and np.delete(stored, list(heavy)).max() <= 6 and np.median(stored) >= 5
    L = rng.integers(0, k, (nb, n))
    rank2, npos, sums, tie, _ = reference_stats(X, L, k)
    with ExpressionMatrix(csr_of(X)) as m:
        out = [m.rank_sum_pass(L, k, which="counts", gather=gather) for gather in ("inplace", "permute")]
    out.append(metrics.rank_sum_pass(X, L, k))                   # the dense entry: the same three genes above the cap
    for r in out:
        assert np.array_equal(r["rank2"], rank2) and np.array_equal(r["npos"], npos) and np.array_equal(r["tie"], tie)
        assert np.allclose(r["sum"], sums, rtol=RTOL, atol=0.0)
        same(out[0], r, "between the handle's gathers and the dense entry")
