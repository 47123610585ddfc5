"""Annotation problems with EXPLICIT pair-marker lists, for the edges of the fine-tuning kernel that the planted cases of
tests/annot_cases.py do not reach.  The lists are given, not derived from medians, so each case chooses its G' (the union of
the lists of the labels in use): its size, where its bits lie in the mask words, whether it is empty.  The marker set M is
all m genes of the case (``pair_masks(pairs, np.arange(m), L)``).

Data rules of every case: the reference holds zeros of both signs (about a tenth of its entries), a few percent negative
values and tie groups (a handful of integer levels through ``log1p``); the cells are ``log1p`` of Poisson counts (zeros and
ties); the labels are interleaved in the caller's order.  A zero in a sample is what the closed-form zero block of the
kernel is for: the planted cases have none.

Every case carries its CPU restatement (tests/annot_reference.py), the trace of the loop (cell, use, |G'| per pass) and is
computed once per process.  tests/test_annot_edge_cases.py shows on the restatement alone that each case is what it claims;
tests/test_gpu_annot_edges.py runs them on the device."""
import functools

import numpy as np

import annot_reference as ar
from scrna_seq_qannealing_clustering_amd import annotate

G_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
CAP_VARIANTS = {"cap_all": 8191, "cap_4097": 4097}


class Case:
    pass


# ---- data ------------------------------------------------------------------------------------------------------------------

def level_profiles(rng, L, m, top=5):
    """L independent profiles of integer levels 1 .. top"""
    return rng.integers(1, top + 1, (L, m)).astype(np.float64)


def near_copy(rng, prof, genes):
    """`prof` with `genes` of its entries moved by two levels, up or down at random (up where down would leave level 1)"""
    out = prof.copy()
    j = rng.choice(prof.size, genes, replace=False)
    down = (rng.random(genes) < 0.5) & (out[j] >= 3)
    out[j] += np.where(down, -2.0, 2.0)
    return out


def reference_rows(rng, prof, noise=0.3, zero_share=0.10, neg_share=0.03):
    """samples of the profile rows `prof`: the level moved by one on a `noise` share of the entries (a number or one per
    row), through log1p; then zeros of both signs on `zero_share` and negative values on `neg_share` of the entries"""
    shape = prof.shape
    lev = prof + rng.integers(-1, 2, shape) * (rng.random(shape) < noise)
    R = np.log1p(np.clip(lev, 1, None))
    u = rng.random(shape)
    R[u < zero_share] = 0.0
    R[u < zero_share / 2] = -0.0
    neg = (u >= zero_share) & (u < zero_share + neg_share)
    R[neg] = -np.log1p(rng.integers(1, 4, shape))[neg]
    return R.astype(np.float32)


def poisson_cells(rng, rate, depth):
    counts = rng.poisson(rate / rate.sum(axis=1, keepdims=True) * depth)
    return np.log1p(counts).astype(np.float32)


def difference_pairs(prof, de_n):
    """pairs[(a, b)]: the `de_n` genes with the largest positive prof[a] - prof[b], ties to the lower index"""
    L = prof.shape[0]
    pairs = {}
    for a in range(L):
        for b in range(L):
            if a != b:
                d = prof[a] - prof[b]
                top = np.argsort(-d, kind="stable")[:de_n]
                pairs[(a, b)] = top[d[top] > 0].astype(np.int64)
    return pairs


def interleaved(rng, sizes):
    return rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)


def finish(c, row_of=None):
    """masks, restatement and trace of a case with X, R, ids, L, pairs; `row_of` as in annot_reference.annotate (c.R then
    holds the distinct rows; full_reference(c) makes the S x m matrix)"""
    c.n, c.m = c.X.shape
    c.S = len(c.ids)
    c.masks = annotate.pair_masks(c.pairs, np.arange(c.m), c.L)
    c.trace = []
    c.expect = ar.annotate(c.X, c.R, c.ids, c.L, c.pairs, trace=c.trace, row_of=row_of)
    for v in c.expect.values():
        v.setflags(write=False)
    c.gsizes = sorted(set(g for _, _, g in c.trace))
    c.row_of = row_of
    for a in (c.X, c.R, c.ids, c.masks):
        a.setflags(write=False)
    return c


def full_reference(c):
    """the S x m reference of a case (built on demand where the case tiles a few rows: 134 MB at the cap, not kept)"""
    return c.R if c.row_of is None else np.ascontiguousarray(c.R[c.row_of])


def uses_of(c, cell):
    """the `use` sets of the passes of one cell, in order"""
    return [use for i, use, _ in c.trace if i == cell]


def step3_margin(sc):
    """the smallest distance of a step-3 decision of every cell: the top-two gap and every |score - (max - 0.05)|"""
    s = np.sort(sc, axis=1)
    gap = s[:, -1] - s[:, -2]
    thr = np.abs(sc - (sc.max(axis=1, keepdims=True) - ar.TUNE_THRESH)).min(axis=1)
    return np.minimum(gap, thr)


# ---- the cases -------------------------------------------------------------------------------------------------------------

def ref_zeros(seed=3):
    """L = 6, label sizes 1 .. 6, m = 700, 60 cells.  Labels 0, 1, 2 are a family (1 a close copy of 0, 2 a more distant
    one: `use` starts with three labels and drops to two), 3 and 4 are near-copies, 5 stands alone (no iteration)."""
    rng = np.random.default_rng(seed)
    L, m, n = 6, 700, 60
    prof = level_profiles(rng, L, m)
    prof[1] = near_copy(rng, prof[0], 10)
    prof[2] = near_copy(rng, prof[0], 45)
    prof[4] = near_copy(rng, prof[3], 14)
    c = Case()
    c.L, c.ids = L, interleaved(rng, [1, 2, 3, 4, 5, 6])
    c.R = reference_rows(rng, prof[c.ids], noise=0.25)
    c.truth = (np.arange(n) % L).astype(np.int32)
    c.X = poisson_cells(rng, prof[c.truth], 1500.0)
    c.pairs = difference_pairs(prof, 60)
    return finish(c)


def big_labels(seed=1):
    """label sizes [3, 70, 300] (S = 373), m = 130, 12 cells; labels 1 and 2 are near-copies, so labels with more than 64 and
    more than 256 samples go through the quantile and through the per-sample loop of the fine-tuning kernel.  The samples
    of label 2 get noisier from first to last, and 40 of them are bit-copies of one whose place among the others puts the
    run of 40 equal rho over the two order statistics of the 0.8 quantile (positions 239 and 240 of 300)."""
    rng = np.random.default_rng(seed)
    sizes, m, n = [3, 70, 300], 130, 12
    prof = level_profiles(rng, 3, m)
    prof[2] = near_copy(rng, prof[1], 10)
    c = Case()
    c.L, c.ids = 3, interleaved(rng, sizes)
    noise = np.full(sum(sizes), 0.3)
    big = np.flatnonzero(c.ids == 2)
    noise[big] = np.linspace(0.05, 0.7, len(big))
    R = reference_rows(rng, prof[c.ids], noise=noise[:, None])
    # 40 clean samples, then the source and its 39 copies, then 220 noisier ones
    c.copies = big[40:80]
    R[c.copies[1:]] = R[c.copies[0]]
    c.R = R
    c.truth = np.array([0, 0, 0] + [1, 2] * 4 + [2], dtype=np.int32)
    c.X = poisson_cells(rng, prof[c.truth], 400.0)
    c.pairs = difference_pairs(prof, 40)
    return finish(c)


def g_genes(k, m=1100):
    """the gene set of size k: gene m - 1 alone, genes 31 and 32 (the word edge) for k = 2, and from k = 63 genes 0, 31, 32
    and m - 1 plus k - 4 others drawn over all words"""
    if k == 1:
        return np.array([m - 1])
    if k == 2:
        return np.array([31, 32])
    rng = np.random.default_rng(1000 + k)
    fixed = np.array([0, 31, 32, m - 1])
    rest = np.setdiff1d(np.arange(m), fixed)
    return np.sort(np.concatenate([fixed, rng.choice(rest, k - 4, replace=False)]))


# seeds for which every cell keeps both labels in use at step 3 and every decision is clear (tests/test_annot_edge_cases.py)
G_SEEDS = {2: 0, 65: 0, 255: 0, 256: 0}


def g_sizes(k, seed=None):
    """L = 2, m = 1100, |G'| = k exactly: the first 60 % of the gene set is the list of (0, 1), the last 60 % that of
    (1, 0), so the lists overlap.  The cells are half-and-half mixtures of the two profiles: both labels are in use at step
    3 for every cell, so every cell makes one pass at least, on G'.
    For k <= 2 every rho is exactly -1, 0 or 1 (k = 1: the cell's da is 0, rho = 0; k = 2: ranks (2, 4) or (3, 3)), so
    scores tie exactly; both implementations give the lower id then, and no margin is asked of these two cases."""
    rng = np.random.default_rng((G_SEEDS.get(k, 1) if seed is None else seed) + 17 * k)
    m, n = 1100, 10
    prof = level_profiles(rng, 2, m)
    prof[1] = near_copy(rng, prof[0], 300)
    c = Case()
    c.k, c.L, c.ids = k, 2, interleaved(rng, [3, 4])
    c.R = reference_rows(rng, prof[c.ids], noise=0.25)
    c.X = poisson_cells(rng, np.tile(prof.mean(axis=0), (n, 1)), 2500.0)
    G = g_genes(k, m)
    cut = max(1, int(np.ceil(0.6 * k)))
    c.genes = G
    c.pairs = {(0, 1): G[:cut], (1, 0): G[k - cut:]}
    return finish(c)


def no_markers(seed=0):
    """labels 0 and 1 are near-copies and BOTH their pair lists are empty; label 2 is distant and has lists against both.
    A cell with use = {0, 1} meets G' = {}: m' = 0, every rho = 0 (da = 0), one pass, the lower id, both tuned scores 0."""
    rng = np.random.default_rng(seed)
    m, n = 200, 16
    prof = level_profiles(rng, 3, m)
    prof[1] = near_copy(rng, prof[0], 6)
    c = Case()
    c.L, c.ids = 3, interleaved(rng, [3, 4, 3])
    c.R = reference_rows(rng, prof[c.ids], noise=0.25)
    c.truth = np.array([0, 1] * 6 + [2] * 4, dtype=np.int32)
    c.X = poisson_cells(rng, prof[c.truth], 600.0)
    c.pairs = difference_pairs(prof, 30)
    c.pairs[(0, 1)] = c.pairs[(1, 0)] = np.empty(0, dtype=np.int64)
    return finish(c)


def duplicate_label(seed=0):
    """label 2's samples are bit-copies of label 1's (the same number, in the same order); label 0 is distant.  The scores of
    1 and 2 are the same integers through the same operations, at step 3 and in every pass: equal exactly."""
    rng = np.random.default_rng(seed)
    m, n = 300, 14
    prof = level_profiles(rng, 2, m)
    c = Case()
    c.L = 3
    c.ids = np.array([1, 0, 2, 1, 2, 0, 1, 0, 2, 1, 2], dtype=np.int32)          # 3, 4 and 4 samples
    R = reference_rows(rng, prof[np.minimum(c.ids, 1)], noise=0.25)
    R[c.ids == 2] = R[c.ids == 1]
    c.R = R
    c.truth = np.array([1] * 10 + [0] * 4, dtype=np.int32)
    c.X = poisson_cells(rng, prof[c.truth], 800.0)
    pr = difference_pairs(prof, 40)
    some = np.sort(rng.choice(m, 70, replace=False))
    c.pairs = {(0, 1): pr[(0, 1)], (1, 0): pr[(1, 0)], (0, 2): pr[(0, 1)], (2, 0): pr[(1, 0)],
               (1, 2): some[:45], (2, 1): some[30:]}
    return finish(c)


def flat_on_g(seed=4):
    """L = 2, five samples each, m = 300, G' = genes 100 .. 199.  The first four cells are non-zero on M but zero on all of
    G' (zeros of both signs): da = 0.  In each label one sample is a non-zero constant on G' and one is zero on G' (both
    signs): db = 0.  (Both labels get both, so that step 3 keeps the two labels within the threshold of each other.)
    rho = 0 by the convention of the specification; a flat cell's scores tie at 0 exactly and the lower id wins."""
    rng = np.random.default_rng(seed)
    m, n = 300, 12
    prof = level_profiles(rng, 2, m)
    prof[1] = near_copy(rng, prof[0], 80)
    c = Case()
    c.L, c.ids = 2, interleaved(rng, [5, 5])
    R = reference_rows(rng, prof[c.ids], noise=0.25)
    c.G = np.arange(100, 200)
    c.const_samples = [int(np.flatnonzero(c.ids == l)[1]) for l in (0, 1)]
    c.zero_samples = [int(np.flatnonzero(c.ids == l)[3]) for l in (0, 1)]
    R[np.ix_(c.const_samples, c.G)] = 1.5
    R[np.ix_(c.zero_samples, c.G)] = np.where(np.arange(100) % 3 == 0, -0.0, 0.0)
    c.R = R
    X = poisson_cells(rng, np.tile(prof.mean(axis=0), (n, 1)), 900.0)
    c.flat = np.arange(4)
    X[np.ix_(c.flat, c.G)] = np.where(np.arange(100) % 2 == 0, -0.0, 0.0)
    c.X = X
    c.pairs = {(0, 1): c.G[:60], (1, 0): c.G[40:]}
    return finish(c)


def cap(genes, seed=0):
    """m = 8191, S = 4096, L = 3: the largest LDS request of the fine-tuning kernel.  Labels 0 and 1 have three samples each
    and are near-copies; label 2 has the other 4090 samples, five distinct rows tiled, and an unrelated profile: it is never
    in use.  The lists of (0, 1) and (1, 0) cover `genes` genes together (all 8191, or 4097: one past a power of two), spread
    over every mask word.  The restatement ranks the 11 distinct rows and indexes them (`row_of`)."""
    rng = np.random.default_rng(seed)
    m, S, n = annotate.MAX_GENES, annotate.MAX_SAMPLES, 6
    prof = level_profiles(rng, 3, m)
    prof[1] = near_copy(rng, prof[0], 600)
    c = Case()
    c.L = 3
    c.ids = np.full(S, 2, dtype=np.int32)
    small = np.sort(rng.choice(S, 6, replace=False))
    c.ids[small] = [0, 1, 1, 0, 1, 0]
    distinct = reference_rows(rng, prof[[0, 1, 1, 0, 1, 0, 2, 2, 2, 2, 2]], noise=0.25)
    row_of = np.empty(S, dtype=np.int64)
    row_of[small] = np.arange(6)
    rest = np.flatnonzero(c.ids == 2)
    row_of[rest] = 6 + np.arange(len(rest)) % 5
    c.R = distinct
    c.truth = np.array([0, 1] * 3, dtype=np.int32)
    c.X = poisson_cells(rng, prof[c.truth], 12000.0)
    G = np.arange(m) if genes == m else np.sort(np.concatenate([[0, m - 1], rng.choice(np.arange(1, m - 1), genes - 2, replace=False)]))
    cut = int(0.6 * genes)
    c.genes = G
    c.pairs = {(0, 1): G[:cut], (1, 0): G[genes - cut:]}
    for l in (0, 1):
        c.pairs[(l, 2)] = c.pairs[(2, l)] = np.empty(0, dtype=np.int64)
    return finish(c, row_of=row_of)


BUILDERS = {"ref_zeros": ref_zeros, "big_labels": big_labels, "no_markers": no_markers, "duplicate_label": duplicate_label,
            "flat_on_g": flat_on_g}
BUILDERS.update({"g_%d" % k: functools.partial(g_sizes, k) for k in G_SIZES})
BUILDERS.update({name: functools.partial(cap, genes) for name, genes in CAP_VARIANTS.items()})
NAMES = list(BUILDERS)
# the cases whose every decision must be clear of rounding on every cell; the others hold engineered exact ties
MARGIN_CHECKED = ["ref_zeros", "big_labels"] + ["g_%d" % k for k in G_SIZES if k >= 63] + list(CAP_VARIANTS)


@functools.lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[name]()
    c.name = name
    return c
