"""Label agreement on the GPU (k_agree_mfma, csrc/agreement_kernels.hip) where the other suite never launches it, on the
cases of tests/agreement_cases.py, every pair against the batched restatement (itself pinned to the scalar one, pair by
pair, in tests/test_agreement_cases.py): more tiles than three full grids of wavefronts at every tile width, in WITHIN mode
(with groups) and in CROSS mode with tables and both operands ending inside a tile; 2 to 6 chunks of cells through the
two-ahead load pipeline; every labelling of 1 to 5 cells, which holds every branch of the closed forms; full 64 x 64 tables
at n = 100 000; and the in-place pass over a padded Potts run at every KB.

``raw`` starts the host outputs as NaN / -1, which shows a copy that did not happen; a pair that no tile wrote comes back as
whatever the device buffer held (zeros or stale bits) and fails the comparison with the restatement, every pair being
compared: a build whose tile loop makes a single pass fails the three past-one-grid tests, every case of them.  Tolerances
are those of test_gpu_agreement.py: tables and pair sums exact, ARI within 1e-12, NMI within 1e-10."""
import numpy as np
import pytest

import agreement_cases as ac
from test_gpu_agreement import WITHIN, padded_run, raw
from scrna_seq_qannealing_clustering_amd import _lib

pytestmark = pytest.mark.gpu

ARI_TOL, NMI_TOL = 1e-12, 1e-10


def compute_units():
    """of device 0, the quantity the launch sizes its grid by"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == _lib.device_info(0)["compute_units"]
    return cus


def check(got, want, what=""):
    """(ari, nmi, S, tables or None) of the device against (tables, S, ari, nmi) of the batched restatement"""
    ari, nmi, S, T = got
    wt, wS, wari, wnmi = want
    assert len(S) == len(wS)
    bad = np.flatnonzero(S != wS)
    assert len(bad) == 0, "%s: %d of %d pair sums differ, first at pair %d: %d, want %d" % (
        what, len(bad), len(S), bad[0], S[bad[0]], wS[bad[0]])
    if T is not None:
        bad = np.flatnonzero((T != wt).any(axis=(1, 2)))
        assert len(bad) == 0, "%s: %d of %d tables differ, first at pair %d:\n%s\nwant\n%s" % (
            what, len(bad), len(S), bad[0], T[bad[0]], wt[bad[0]])
    # (a NaN fails both: the comparisons are written so that NaN is not <=)
    da, dn = np.abs(ari - wari), np.abs(nmi - wnmi)
    assert (da <= ARI_TOL).all(), "%s: ARI off by %g at pair %d" % (what, np.nanmax(da), int(np.argmax(~(da <= ARI_TOL))))
    assert (dn <= NMI_TOL).all(), "%s: NMI off by %g at pair %d" % (what, np.nanmax(dn), int(np.argmax(~(dn <= NMI_TOL))))


# ---- a. WITHIN past one grid ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("K", ac.WITHIN_K)
def test_within_past_one_grid(K, G):
    cus = compute_units()
    A = ac.within_case(K, G, cus)
    Rg = ac.within_rows(K, G, cus)
    tiles, waves, passes = ac.launch(G * Rg, 0, K, K, G, cus, within=True)
    print("within K=%d G=%d: Rg=%d, %d tiles on %d wavefronts (%d CUs), >= %d passes each" % (K, G, Rg, tiles, waves, cus, passes))
    assert tiles >= 3 * 4 * cus and waves == 4 * cus and passes >= 3
    assert A.shape == (G * Rg, 130) and Rg % ac.tile_width(K, K) == 1 % ac.tile_width(K, K)
    got = raw(A, None, K, K, WITHIN, G, tables=False)
    check(got, ac.expected(A, A, K, K, ac.within_pairs(Rg, G)), "within K=%d G=%d" % (K, G))
    if G > 1:                                                        # the group layout: each group is its own G = 1 call
        P = Rg * (Rg - 1) // 2
        for g in range(G):
            one = raw(A[g * Rg:(g + 1) * Rg], None, K, K, WITHIN, 1, tables=False)
            for x, y in zip(got[:3], one[:3]):
                assert np.array_equal(x[g * P:(g + 1) * P], y)


# ---- b. CROSS past one grid, with tables ----------------------------------------------------------------------------

@pytest.mark.parametrize("Ka,Kb", ac.CROSS_K)
def test_cross_past_one_grid_with_tables(Ka, Kb):
    cus = compute_units()
    A, B = ac.cross_case(Ka, Kb, cus)
    Ra, Rb = len(A), len(B)
    tiles, waves, passes = ac.launch(Ra, Rb, Ka, Kb, 1, cus, within=False)
    print("cross Ka=%d Kb=%d: %d x %d, %d tiles on %d wavefronts (%d CUs), >= %d passes each" % (Ka, Kb, Ra, Rb, tiles, waves, cus, passes))
    assert tiles >= 3 * 4 * cus and waves == 4 * cus and passes >= 3
    assert Ra * Rb * Ka * Kb <= (1 << 28) // 16                      # well under MI_AGREE_MAX_TABLE_ENTRIES
    T = ac.tile_width(Ka, Kb)
    assert Ra != Rb and Ra % T in (1 % T, 3 % T) and Rb % T in (1 % T, 3 % T)
    check(raw(A, B, Ka, Kb), ac.expected(A, B, Ka, Kb, ac.cross_pairs(Ra, Rb)), "cross %d x %d" % (Ka, Kb))


# ---- c. the chunk pipeline ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Ka,Kb", ac.CHUNK_K)
@pytest.mark.parametrize("n", ac.CHUNK_N)
def test_chunk_pipeline_exact_tables(n, Ka, Kb):
    """a table's entries sum to n: a chunk dropped, counted twice or taken from the other buffer cannot pass"""
    A, B = ac.chunk_case(n, Ka, Kb)
    check(raw(A, B, Ka, Kb), ac.expected(A, B, Ka, Kb, ac.cross_pairs(5, 3)), "n=%d (%d chunks)" % (n, ac.chunks(n)))


@pytest.mark.parametrize("Ka,Kb", ac.CHUNK_K)
@pytest.mark.parametrize("n", ac.CHUNK_N)
def test_chunk_pipeline_labels_name_the_chunk(n, Ka, Kb):
    """cell i has label (i // 64 + r) % Ka in row r of A and (7 (i // 64) + r) % Kb in row r of B: a wrong entry names the chunk"""
    A, B = ac.chunk_index_case(n, Ka, Kb)
    check(raw(A, B, Ka, Kb), ac.expected(A, B, Ka, Kb, ac.cross_pairs(5, 3)), "n=%d (%d chunks)" % (n, ac.chunks(n)))


# ---- d. every labelling of a few cells ------------------------------------------------------------------------------

@pytest.mark.parametrize("n", ac.SMALL_N)
def test_every_labelling_of_a_few_cells(n):
    L = ac.every_labelling(n)
    R = len(L)
    pairs = ac.cross_pairs(R, R)
    got = raw(L, L, 3, 3)
    check(got, ac.expected(L, L, 3, 3, pairs), "every labelling, n=%d, cross" % n)
    if n == 5:
        cus = compute_units()
        tiles, waves, passes = ac.launch(R, R, 3, 3, 1, cus, within=False)
        print("every labelling of 5 cells: %d x %d, %d tiles on %d wavefronts (%d CUs)" % (R, R, tiles, waves, cus))
        assert tiles == 3721 and tiles >= 3 * 4 * cus and passes >= 3
    ari, nmi, S, _ = got
    cls, const = ac.small_classes(L)
    i, j = pairs[:, 0], pairs[:, 1]
    relabelled = cls[i] == cls[j]
    assert relabelled.sum() >= R and (ari[relabelled] == 1.0).all() and (nmi[relabelled] == 1.0).all()
    assert (ari[~relabelled] < 1.0).all()
    one_const = const[i] ^ const[j]
    assert (nmi[one_const] == 0.0).all() and one_const.sum() == (2 * 3 * (R - 3) if n > 1 else 0)
    both = const[i] & const[j]
    assert both.sum() == 9 and (ari[both] == 1.0).all() and (nmi[both] == 1.0).all()
    if n == 1:
        assert (ari == 1.0).all() and (nmi == 1.0).all() and (S == 0).all()
    # WITHIN, one group: the pairs r < s of the same set
    wp = ac.within_pairs(R)
    wgot = raw(L, None, 3, 3, WITHIN, 1, tables=False)
    check(wgot, ac.expected(L, L, 3, 3, wp), "every labelling, n=%d, within" % n)
    flat = wp[:, 0] * R + wp[:, 1]
    for x, y in zip(wgot[:3], got[:3]):
        assert np.array_equal(x, y[flat])                             # WITHIN is the upper triangle of CROSS, bit for bit


# ---- e. large n, full tables ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("Ka,Kb", ac.LARGE_K)
def test_large_n_full_tables(Ka, Kb):
    A, B = ac.large_case(Ka, Kb)
    pairs = ac.cross_pairs(5, 5)
    got = raw(A, B, Ka, Kb)
    want = ac.expected(A, B, Ka, Kb, pairs)
    check(got, want, "n=100000 %d x %d" % (Ka, Kb))
    ari, nmi, S, T = got
    assert (T[0] > 0).all() and (T[18] > 0).all() and (T[24] > 0).all()           # independent rows fill the table
    assert S[6] > 2 ** 31 and S[6] == want[1][6]                      # the near-identical pair
    assert ari[12] == 1.0 and abs(nmi[12] - 1.0) <= 1e-12             # B[2] is A[2] relabelled


# ---- f. in place over a padded Potts run, at every KB ---------------------------------------------------------------

@pytest.mark.parametrize("K", [16, 32, 64])
def test_in_place_on_a_padded_run_at_every_label_block_count(K):
    """padded_run asserts that the layout has holes (p.n_dev > pm.num_variables); the graph's layout does not depend on K"""
    st, en, agree, agree2 = padded_run(True, K)
    st0, en0, _, _ = padded_run(False, K)
    assert np.array_equal(st, st0) and np.array_equal(en, en0)
    print("in place K=%d: labels used up to %d" % (K, st.max()))
    assert st.max() >= K - 16                                         # the last block of 16 label rows is in use
    ari, nmi, S, _ = raw(st, None, K, K, WITHIN, 3, tables=False)
    assert agree2["ari"].shape == (3, 28)
    assert np.array_equal(agree2["pair_sum"].ravel(), S)
    assert np.allclose(agree2["ari"].ravel(), ari, rtol=0, atol=1e-13)
    assert np.allclose(agree2["nmi"].ravel(), nmi, rtol=0, atol=1e-13)
    assert agree["ari"].shape == (1, 24 * 23 // 2)
    check((ari, nmi, S, None), ac.expected(st, st, K, K, ac.within_pairs(8, 3)), "in place K=%d" % K)
