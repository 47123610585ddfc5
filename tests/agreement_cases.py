"""The edge cases of label agreement (k_agree_mfma, csrc/agreement_kernels.hip) and a batched form of the restatement,
shared by tests/test_agreement_cases.py, which pins the batched form to the scalar one of tests/test_agreement_model.py and
shows on the CPU that every case reaches what it is meant to reach (tile counts past one grid, chunk counts, the degenerate
pairs), and tests/test_gpu_agreement_edges.py, which holds the device to it.  TEST INFRASTRUCTURE ONLY.

The scalar restatement costs 0.2 ms (K = 16) to 1.6 ms (K = 64) per pair; the cases below have tens of thousands of pairs.
``batch_tables`` counts the tables of a block of pairs with one bincount, ``batch_agreement`` evaluates ref_ari's and
ref_nmi's formulas, special cases included, on all tables at once.

The launch of k_agree_mfma (mi_label_agreement_dev): 4 wavefronts per workgroup, min(ceil(tiles / 4), CUs) workgroups, every
wavefront on tiles w, w + 4 blocks, ...; a tile is T x T labellings, T = 4 / KB, KB = 1, 2, 4 for max(Ka, Kb) <= 16, 32, 64.
``launch`` restates that, so a case can say how often a wavefront goes round its loop."""
import functools
import itertools
import math

import numpy as np

BLOCK_BYTES = 100 << 20          # of int64 work arrays per block of pairs in batch_tables
WAVES = 4                        # kAgreeWaves
GRID_PASSES = 3                  # what "past one grid" asks: every wavefront of a full grid goes round at least this often
CUS_MI355X = 256


# ---- the batched restatement ----------------------------------------------------------------------------------------

def batch_tables(A, B, Ka, Kb, pairs):
    """Exact contingency tables, int64 [P, Ka, Kb], of the pairs (row i of A, row j of B) for (i, j) in ``pairs`` [P, 2]."""
    A, B = np.asarray(A, dtype=np.int64), np.asarray(B, dtype=np.int64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    n, P, KK = A.shape[1], len(pairs), Ka * Kb
    assert B.shape[1] == n and A.min() >= 0 and A.max() < Ka and B.min() >= 0 and B.max() < Kb
    out = np.empty((P, Ka, Kb), dtype=np.int64)
    step = max(1, BLOCK_BYTES // (8 * max(KK, n)))
    for p0 in range(0, P, step):
        blk = pairs[p0:p0 + step]
        key = (np.arange(len(blk))[:, None] * KK + A[blk[:, 0]] * Kb) + B[blk[:, 1]]
        out[p0:p0 + len(blk)] = np.bincount(key.ravel(), minlength=len(blk) * KK).reshape(len(blk), Ka, Kb)
    assert (out.sum(axis=(1, 2)) == n).all()
    return out


def _comb2(c):
    return (c * (c - 1) // 2).sum(axis=-1)


def _ln(c):
    """ln c for c > 0 and 0 for c = 0 (every use multiplies it by c): no log of zero is taken"""
    return np.log(np.where(c > 0, c, 1).astype(np.float64))


def batch_agreement(tables, n):
    """``S`` (int64, exact), ``ari`` and ``nmi`` (fp64) of every table of ``tables`` [P, Ka, Kb] over n cells: ref_ari's and
    ref_nmi's formulas and special cases (tests/test_agreement_model.py), evaluated for all tables at once."""
    t = np.asarray(tables, dtype=np.int64)
    P = t.shape[0]
    ra, rb = t.sum(axis=2), t.sum(axis=1)
    S, a, b = _comb2(t.reshape(P, -1)), _comb2(ra), _comb2(rb)
    # ARI: 1.0 when S == a == b, 1.0 when den == 0
    same = (S == a) & (S == b)
    c2 = n * (n - 1) / 2.0
    one = np.ones(P)
    p = np.divide(a.astype(np.float64) * b.astype(np.float64), c2, out=np.zeros(P), where=~same)     # (n = 1: every pair is `same`)
    den = 0.5 * (a + b) - p
    flat = same | (den == 0)
    ari = np.where(flat, 1.0, np.divide(S - p, den, out=one.copy(), where=~flat))
    # NMI: 1.0 / 0.0 with a single cluster on both sides / one side, MI clipped at 0
    ka, kb = (ra > 0).sum(axis=1), (rb > 0).sum(axis=1)
    term = t / n * (_ln(t) + math.log(n) - _ln(ra)[:, :, None] - _ln(rb)[:, None, :])
    mi = np.maximum(term.reshape(P, -1).sum(axis=1), 0.0)
    fa, fb = ra / n, rb / n
    ha, hb = -(fa * _ln2(fa)).sum(axis=1), -(fb * _ln2(fb)).sum(axis=1)
    mean = 0.5 * (ha + hb)
    live = (ka > 1) & (kb > 1) & (mi > 0.0)
    nmi = np.where(live, np.divide(mi, mean, out=one.copy(), where=live), 0.0)
    nmi = np.where((ka == 1) & (kb == 1), 1.0, nmi)
    assert np.isfinite(ari).all() and np.isfinite(nmi).all() and (S >= 0).all()
    return S, ari, nmi


def _ln2(f):
    """ln f for f > 0 and 0 for f = 0, for fractions"""
    return np.log(np.where(f > 0, f, 1.0))


def cross_pairs(Ra, Rb):
    """the pairs of a CROSS call in its output order"""
    return np.stack(np.meshgrid(np.arange(Ra), np.arange(Rb), indexing="ij"), axis=-1).reshape(-1, 2)


def within_pairs(Rg, G=1):
    """the pairs r < s of a WITHIN call in its output order (rows of the whole array)"""
    iu = np.stack(np.triu_indices(Rg, 1), axis=-1)
    return np.concatenate([iu + g * Rg for g in range(G)])


def expected(A, B, Ka, Kb, pairs):
    """(tables, S, ari, nmi) of the batched restatement"""
    t = batch_tables(A, B, Ka, Kb, pairs)
    return (t,) + batch_agreement(t, np.asarray(A).shape[1])


# ---- the launch -----------------------------------------------------------------------------------------------------

def tile_width(Ka, Kb):
    K = max(Ka, Kb)
    return 4 if K <= 16 else (2 if K <= 32 else 1)


def launch(Ra, Rb, Ka, Kb, G, cus, within):
    """(tiles, wavefronts of the grid, fewest loop passes of any wavefront) of the call"""
    T = tile_width(Ka, Kb)
    if within:
        nb = -(-(Ra // G) // T)
        tiles = G * nb * (nb + 1) // 2
    else:
        tiles = -(-Ra // T) * -(-Rb // T)
    waves = WAVES * min(-(-tiles // WAVES), cus)
    return tiles, waves, tiles // waves


def chunks(n):
    return -(-n // 64)


# ---- the cases ------------------------------------------------------------------------------------------------------

def near(rng, truth, K, p):
    out = truth.copy()
    flip = rng.random(truth.shape) < p
    out[flip] = rng.integers(0, K, int(flip.sum()))
    return out


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# a. WITHIN past one grid: Rg one more than a multiple of T, nb(nb + 1) / 2 * G tiles >= GRID_PASSES * 4 * CUs
WITHIN_N = 130                   # three chunks, the last partial
WITHIN_K = (16, 32, 64)


def within_rows(K, G, cus=CUS_MI355X):
    """Rg of the case: nb tile rows with G nb (nb + 1) / 2 >= GRID_PASSES * WAVES * cus, at least the 81 (G = 1) / 58 (G = 2)
    that do on 256 CUs with room, and Rg = T (nb - 1) + 1"""
    nb = 81 if G == 1 else 58
    while G * nb * (nb + 1) // 2 < GRID_PASSES * WAVES * cus:
        nb += 1
    return tile_width(K, K) * (nb - 1) + 1


@functools.lru_cache(maxsize=None)
def within_case(K, G, cus=CUS_MI355X):
    """[G Rg, 130] labellings: noisy copies of one truth, noise 0 .. 0.5 by row; in every group the last row (alone in its
    tile row) repeats the first, and the middle row is a single cluster"""
    Rg = within_rows(K, G, cus)
    rng = np.random.default_rng(1000 * K + G)
    truth = rng.integers(0, K, WITHIN_N)
    A = np.stack([near(rng, truth, K, 0.5 * (r % Rg) / (Rg - 1)) for r in range(G * Rg)])
    for g in range(G):
        A[g * Rg + Rg - 1] = A[g * Rg]
        A[g * Rg + Rg // 2] = K - 1
    return _ro(A.astype(np.uint16))


# b. CROSS past one grid, with tables
CROSS_N = 70
CROSS_K = ((16, 9), (17, 32), (64, 17))


def cross_rows(Ka, Kb, cus=CUS_MI355X):
    """(Ra, Rb): both one or three more than a multiple of T, different, ceil(Ra / T) ceil(Rb / T) >= GRID_PASSES * WAVES * cus;
    259 x 257, 131 x 129, 67 x 66 on 256 CUs"""
    T = tile_width(Ka, Kb)
    m = 65
    while m * m < GRID_PASSES * WAVES * cus:
        m += 1
    if T == 4:
        return 4 * (m - 1) + 3, 4 * (m - 1) + 1
    if T == 2:
        return 2 * m + 1, 2 * (m - 1) + 1
    return m + 2, m + 1


@functools.lru_cache(maxsize=None)
def cross_case(Ka, Kb, cus=CUS_MI355X):
    """(A [Ra, 70], B [Rb, 70]): noisy copies of one truth (mod K on each side); the last row of B (in a partial tile) never
    uses label Kb - 1, and the last row of A is a single cluster"""
    Ra, Rb = cross_rows(Ka, Kb, cus)
    rng = np.random.default_rng(100 * Ka + Kb)
    truth = rng.integers(0, 64, CROSS_N)
    A = np.stack([near(rng, truth % Ka, Ka, 0.5 * r / (Ra - 1)) for r in range(Ra)])
    B = np.stack([near(rng, truth % Kb, Kb, 0.5 * r / (Rb - 1)) for r in range(Rb)])
    B[Rb - 1] = np.minimum(B[Rb - 1], Kb - 2)
    A[Ra - 1] = Ka // 2
    return _ro(A.astype(np.uint16), B.astype(np.uint16))


# c. the chunk pipeline
CHUNK_N = (127, 128, 129, 191, 192, 193, 255, 257, 320, 321)
CHUNK_NCH = (2, 2, 3, 3, 3, 4, 4, 5, 5, 6)
CHUNK_K = ((16, 13), (32, 29), (64, 61))         # (Ka, Kb): K = 16, 32, 64 with Ka != Kb


@functools.lru_cache(maxsize=None)
def chunk_case(n, Ka, Kb):
    """(A [5, n], B [3, n]) random near a truth, as test_gpu_agreement.py:test_cross_exact"""
    rng = np.random.default_rng(n * 131 + Ka * 7 + Kb)
    A = np.stack([rng.integers(0, Ka - (r % 2), n) for r in range(5)])
    B = np.stack([near(rng, A[r] % Kb, Kb - (r % 2), 0.3) for r in range(3)])
    return _ro(A.astype(np.uint16), B.astype(np.uint16))


@functools.lru_cache(maxsize=None)
def chunk_index_case(n, Ka, Kb):
    """(A [5, n], B [3, n]): the labels of cell i are a function of its chunk i // 64 alone, (c + r) % Ka in row r of A and
    (7 c + r) % Kb in row r of B, so a table entry names the chunks it counts"""
    c = np.arange(n) // 64
    A = np.stack([(c + r) % Ka for r in range(5)])
    B = np.stack([(c * 7 + r) % Kb for r in range(3)])
    return _ro(A.astype(np.uint16), B.astype(np.uint16))


# d. every labelling of a few cells
SMALL_K = 3
SMALL_N = (1, 2, 3, 4, 5)


@functools.lru_cache(maxsize=None)
def every_labelling(n):
    """[3^n, n]: all labellings of n cells with 3 labels, in counting order (row 0 all zero)"""
    return _ro(np.array(list(itertools.product(range(SMALL_K), repeat=n)), dtype=np.uint16))


def canonical(L):
    """every row relabelled by first occurrence: two rows are relabellings of each other iff these are equal"""
    L = np.asarray(L, dtype=np.int64)
    out = np.empty_like(L)
    for r, row in enumerate(L):
        _, first, inv = np.unique(row, return_index=True, return_inverse=True)
        out[r] = np.argsort(np.argsort(first))[inv]
    return out


def small_classes(L):
    """(class id of every row by ``canonical``, whether the row is constant)"""
    can = canonical(L)
    _, cls = np.unique(can, axis=0, return_inverse=True)
    return cls.ravel(), (can.max(axis=1) == 0)


# e. large n, full tables
LARGE_N = 100000
LARGE_K = ((64, 64), (17, 33))


@functools.lru_cache(maxsize=None)
def large_case(Ka, Kb):
    """(A [5, n], B [5, n]) at n = 100 000.  Rows 0, 3, 4: independent uniform labels on both sides (every entry of the table
    is used).  Row 1: one cluster with 70 % of the cells and the rest uniform over all labels; B[1] is A[1] with 1 % of the
    cells moved, so that pair's S passes 2^31.  B[2] is A[2] under an injective relabelling."""
    rng = np.random.default_rng(7 * Ka + Kb)
    n, Km = LARGE_N, min(Ka, Kb)
    A = np.stack([rng.integers(0, Ka, n) for _ in range(5)])
    B = np.stack([rng.integers(0, Kb, n) for _ in range(5)])
    skew = np.where(rng.random(n) < 0.7, 3, rng.integers(0, Km, n))
    A[1] = skew
    B[1] = skew
    moved = rng.choice(n, n // 100, replace=False)
    B[1, moved] = (skew[moved] + 1 + rng.integers(0, Km - 1, len(moved))) % Km      # another label for each
    B[2] = rng.permutation(Kb)[:Ka][A[2]]
    return _ro(A.astype(np.uint16), B.astype(np.uint16))
