"""tests/agreement_cases.py without a GPU: the batched restatement equals the scalar one of tests/test_agreement_model.py
(tables bit for bit, S exactly, ARI and NMI to the summation order) on every pair of the exhaustive small set, which holds
every special case, on a mixed set with Ka != Kb and unused labels, and on sampled pairs of each large case; and every case
reaches what tests/test_gpu_agreement_edges.py runs it for, so that a GPU run cannot pass vacuously."""
import numpy as np
import pytest

import agreement_cases as ac
from test_agreement_model import ref_ari, ref_contingency, ref_nmi, ref_pair_sum

TOL = 1e-13                      # both sides are fp64 evaluations of one formula: only the order of the sums differs


def scalar(A, B, pairs):
    S = np.array([ref_pair_sum(A[i], B[j]) for i, j in pairs], dtype=np.int64)
    ari = np.array([ref_ari(A[i], B[j]) for i, j in pairs])
    nmi = np.array([ref_nmi(A[i], B[j]) for i, j in pairs])
    return S, ari, nmi


def check_against_scalar(A, B, Ka, Kb, pairs):
    t, S, ari, nmi = ac.expected(A, B, Ka, Kb, pairs)
    wS, wari, wnmi = scalar(A, B, pairs)
    assert np.array_equal(S, wS)
    assert np.abs(ari - wari).max() <= TOL and np.abs(nmi - wnmi).max() <= TOL
    return t, S, ari, nmi


def sample(pairs, count, seed):
    pairs = np.asarray(pairs)
    return pairs[np.sort(np.random.default_rng(seed).choice(len(pairs), min(count, len(pairs)), replace=False))]


# ---- 1. the batched restatement -------------------------------------------------------------------------------------

def test_batch_tables_equal_ref_contingency_on_a_mixed_set():
    rng = np.random.default_rng(2)
    for n, Ka, Kb in ((1, 2, 3), (70, 16, 9), (130, 17, 64), (321, 64, 2), (65, 5, 5)):
        A = np.stack([rng.integers(0, max(Ka - (r % 3), 1), n) for r in range(7)])          # top labels unused in some rows
        B = np.stack([rng.integers(0, max(Kb - 2 * (r % 2), 1), n) for r in range(4)])
        pairs = ac.cross_pairs(7, 4)
        t = ac.batch_tables(A, B, Ka, Kb, pairs)
        assert t.dtype == np.int64 and t.shape == (28, Ka, Kb)
        for p, (i, j) in enumerate(pairs):
            assert np.array_equal(t[p], ref_contingency(A[i], B[j], Ka, Kb)), (n, i, j)
        assert (t[:, Ka - 1, :].sum(axis=1) == 0).any() or Ka <= 2
        check_against_scalar(A, B, Ka, Kb, pairs)


def test_batch_tables_blocks_do_not_change_the_result(monkeypatch):
    A, B = ac.chunk_case(193, 16, 13)
    pairs = ac.cross_pairs(5, 3)
    whole = ac.batch_tables(A, B, 16, 13, pairs)
    monkeypatch.setattr(ac, "BLOCK_BYTES", 8 * 16 * 13 * 4)          # four pairs per block: 4 + 4 + 4 + 3
    assert np.array_equal(ac.batch_tables(A, B, 16, 13, pairs), whole)


@pytest.mark.parametrize("n", ac.SMALL_N)
def test_batch_agreement_on_every_pair_of_every_labelling(n):
    """every special case is here: S == a == b (relabellings), one or both sides constant, MI clipped at 0 (independent
    labellings, e.g. 0011 against 0101), den == 0 never without S == a == b, n = 1"""
    L = ac.every_labelling(n)
    assert L.shape == (3 ** n, n)
    pairs = ac.cross_pairs(len(L), len(L))
    t, S, ari, nmi = check_against_scalar(L, L, 3, 3, pairs)
    cls, const = ac.small_classes(L)
    i, j = pairs[:, 0], pairs[:, 1]
    relabelled = cls[i] == cls[j]
    # (the restatement's NMI of a relabelling is MI / H with MI and H summed differently: 1 to a rounding, not 1.0; the
    # device divides two identical expressions and is held to 1.0 in tests/test_gpu_agreement_edges.py)
    assert np.array_equal(relabelled, ari == 1.0) and np.abs(nmi[relabelled] - 1.0).max() <= TOL
    assert (nmi[~relabelled] < 1.0 - 1e-3).all()
    assert (nmi[const[i] ^ const[j]] == 0.0).all() and (nmi[const[i] & const[j]] == 1.0).all()
    if n == 1:
        assert (ari == 1.0).all() and (nmi == 1.0).all() and (S == 0).all()
    if n == 4:
        assert ((nmi == 0.0) & ~const[i] & ~const[j]).any()           # 0011 against 0101: MI is 0 with two clusters on both sides
    if n >= 4:
        assert (ari < 0).any()


# ---- 2. the cases meet their conditions -----------------------------------------------------------------------------

@pytest.mark.parametrize("cus", [256, 304])
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("K", ac.WITHIN_K)
def test_within_cases_go_round_the_tile_loop(K, G, cus):
    T = ac.tile_width(K, K)
    Rg = ac.within_rows(K, G, cus)
    tiles, waves, passes = ac.launch(G * Rg, 0, K, K, G, cus, within=True)
    assert Rg % T == 1 % T and waves == 4 * cus and tiles >= 3 * 4 * cus and passes >= 3
    if cus == 256:
        assert Rg == {(16, 1): 321, (32, 1): 161, (64, 1): 81, (16, 2): 229, (32, 2): 115, (64, 2): 58}[K, G]
        assert tiles == (3321 if G == 1 else 3422)


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("K", ac.WITHIN_K)
def test_within_cases_hold_their_rows_and_match_the_scalar_restatement(K, G):
    A = ac.within_case(K, G)
    Rg = ac.within_rows(K, G)
    assert A.shape == (G * Rg, 130) and ac.chunks(130) == 3 and 130 % 64 != 0
    assert A.max() == K - 1 and ac.tile_width(K, K) == {16: 4, 32: 2, 64: 1}[K]
    for g in range(G):
        blk = A[g * Rg:(g + 1) * Rg]
        assert np.array_equal(blk[0], blk[Rg - 1]) and len(np.unique(blk[Rg // 2])) == 1
        noise = (blk != blk[0]).mean(axis=1)
        assert noise[1] < 0.05 and noise[Rg - 2] > 0.35
    check_against_scalar(A, A, K, K, sample(ac.within_pairs(Rg, G), 300, K + G))


@pytest.mark.parametrize("cus", [256, 304])
@pytest.mark.parametrize("Ka,Kb", ac.CROSS_K)
def test_cross_cases_go_round_the_tile_loop(Ka, Kb, cus):
    T = ac.tile_width(Ka, Kb)
    Ra, Rb = ac.cross_rows(Ka, Kb, cus)
    tiles, waves, passes = ac.launch(Ra, Rb, Ka, Kb, 1, cus, within=False)
    assert Ra != Rb and Ra % T in (1 % T, 3 % T) and Rb % T in (1 % T, 3 % T)
    assert waves == 4 * cus and tiles >= 3 * 4 * cus and passes >= 3
    assert Ra * Rb * Ka * Kb * 4 <= 40 << 20                          # bytes of tables, far below MI_AGREE_MAX_TABLE_ENTRIES
    if cus == 256:
        assert (Ra, Rb) == {4: (259, 257), 2: (131, 129), 1: (67, 66)}[T]


@pytest.mark.parametrize("Ka,Kb", ac.CROSS_K)
def test_cross_cases_hold_their_rows_and_match_the_scalar_restatement(Ka, Kb):
    A, B = ac.cross_case(Ka, Kb)
    assert (A.shape, B.shape) == tuple((r, 70) for r in ac.cross_rows(Ka, Kb)) and ac.chunks(70) == 2
    assert A.max() == Ka - 1 and B[:-1].max() == Kb - 1 and B[-1].max() < Kb - 1 and len(np.unique(A[-1])) == 1
    pairs = sample(ac.cross_pairs(len(A), len(B)), 300, Ka)
    last = np.array([[len(A) - 1, 0], [len(A) - 1, len(B) - 1], [0, len(B) - 1]])
    check_against_scalar(A, B, Ka, Kb, np.concatenate([pairs, last]))


def test_chunk_cases_cover_two_to_six_chunks_with_both_parities():
    assert tuple(ac.chunks(n) for n in ac.CHUNK_N) == ac.CHUNK_NCH == (2, 2, 3, 3, 3, 4, 4, 5, 5, 6)
    assert [ac.tile_width(*k) for k in ac.CHUNK_K] == [4, 2, 1] and all(ka != kb for ka, kb in ac.CHUNK_K)
    for Ka, Kb in ac.CHUNK_K:
        for n in (129, 321):
            A, B = ac.chunk_case(n, Ka, Kb)
            assert A.shape == (5, n) and B.shape == (3, n) and A.max() == Ka - 1 and B.max() == Kb - 1
            check_against_scalar(A, B, Ka, Kb, ac.cross_pairs(5, 3))
            A, B = ac.chunk_index_case(n, Ka, Kb)
            t = ac.batch_tables(A, B, Ka, Kb, ac.cross_pairs(5, 3))
            # pair (0, 0): chunk c alone fills entry (c % Ka, 7 c % Kb), with its 64 cells (fewer in the last chunk)
            want = np.zeros((Ka, Kb), dtype=np.int64)
            for c in range(ac.chunks(n)):
                want[c % Ka, 7 * c % Kb] += min(64, n - 64 * c)
            assert np.array_equal(t[0], want) and (want > 0).sum() == ac.chunks(n)


@pytest.mark.parametrize("Ka,Kb", ac.LARGE_K)
def test_large_cases_fill_the_table_and_pass_int32(Ka, Kb):
    A, B = ac.large_case(Ka, Kb)
    assert A.shape == B.shape == (5, 100000)
    pairs = ac.cross_pairs(5, 5)
    t, S, ari, nmi = check_against_scalar(A, B, Ka, Kb, pairs)
    for r in (0, 3, 4):
        assert (t[r * 5 + r] > 0).all()                               # independent uniform rows: every entry of Ka x Kb
    assert S[1 * 5 + 1] > 2 ** 31 and 0.9 < ari[6] < 1.0 and (A[1] != B[1]).sum() == 1000
    assert len(np.unique(A[1])) == min(Ka, Kb)
    assert ari[2 * 5 + 2] == 1.0 and abs(nmi[12] - 1.0) <= 1e-12 and not np.array_equal(A[2], B[2])
    assert np.abs(ari[[0, 18, 24]]).max() < 1e-3
