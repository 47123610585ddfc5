"""Cell-type annotation on the GPU at the edges tests/test_gpu_annot.py does not reach: more than one 64-sample tile in
the cross pass (S up to 257, interleaved labels), the grid cap of the cross pass and a second chunk into buffers reserved
larger, labels of more than 256 samples and equal rho inside a label in the quantile, S = 4096 with L = 64, and the
fine-tuning kernel on the cases of tests/annot_edge_cases.py: references full of zeros (the closed-form zero block), G' of
0, 1, 2 and 63 .. 1025 genes and of 4097 and 8191 genes at S = 4096 (the largest LDS request), exact ties, flat cells and
samples.  Integers with ``np.array_equal``, scores bit for bit, labels and iteration counts on every cell
(tests/test_annot_edge_cases.py shows the margins).  Then handle reuse, and the rule that a refused ``mi_annot_score``
leaves no resident chunk."""
import ctypes as C

import numpy as np
import pytest

import annot_edge_cases as ec
import annot_reference as ar
from scrna_seq_qannealing_clustering_amd import _lib, annotate

pytestmark = pytest.mark.gpu

KEYS = ("scores", "first_labels", "iterations", "labels", "tuned_best", "tuned_next")


def rows(rng, r, m, zeros=0.3, negatives=0.05):
    """rows with zeros, ties (small counts through log1p, a scale per row) and some negative values: asymmetric data"""
    x = np.log1p(rng.integers(1, 6, (r, m)) * rng.choice([0.5, 1.0, 2.0], (r, 1)))
    x[rng.random((r, m)) < negatives] *= -1.0
    x[rng.random((r, m)) < zeros] = 0.0
    return x.astype(np.float32)


def interleaved(rng, sizes):
    return rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)


def assert_integers(r, sab, sa2, sb2):
    assert r["sab"].shape == sab.shape and r["sab"].dtype == np.int64
    assert np.array_equal(r["sa2"], sa2), "sum a^2"
    assert np.array_equal(r["sb2"], sb2), "sum b^2"
    assert np.array_equal(r["sab"], sab), "sum a b"


# ---- 1. the cross pass -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [63, 64, 65, 127, 128, 129, 257])
@pytest.mark.parametrize("n", [1, 17, 33])
def test_integers_past_one_sample_tile(n, S):
    """ts = ceil(S / 64) > 1 from S = 65: tiles t -> (ti, tj) with tj > 0, the clamp of a partial last sample tile, and the
    column un-permutation of interleaved labels past one tile"""
    rng = np.random.default_rng(1000 * n + S)
    X, R = rows(rng, n, 65), rows(rng, S, 65, zeros=0.1)
    labels = interleaved(rng, [S - 2 * (S // 3), S // 3, S // 3])
    r = annotate.score_pass(X, R, labels=labels)
    assert_integers(r, *ar.integers(X, R))


def test_cross_pass_past_the_grid_cap_and_a_one_cell_chunk():
    """n = 16 385 with the default chunk: one full chunk of 16 384 cells (1024 cell tiles), then one cell into buffers
    reserved for 16 384.  S is chosen from the CU count so that the full chunk has more tiles than the 32 * CUs the capped
    grid (8 * CUs workgroups of four wavefronts) covers in one sweep: the grid stride of k_annot_cross runs."""
    cus = _lib.device_info(0)["compute_units"]
    ts = 32 * cus // 1024 + 1
    S, m, n = 64 * (ts - 1) + 17, 64, annotate.MAX_CHUNK + 1
    assert 1024 * ts > 32 * cus and S <= annotate.MAX_SAMPLES, (cus, ts, S)
    sizes = [7, (S - 7) // 2, S - 7 - (S - 7) // 2]
    assert min(sizes[1:]) > 256, sizes
    rng = np.random.default_rng(16385)
    X, R = rows(rng, n, m), rows(rng, S, m, zeros=0.1)
    labels = interleaved(rng, sizes)
    r = annotate.score_pass(X, R, labels=labels)
    # every partial sum is at most 64 * 128^2 = 2^20: the float64 product of the doubled ranks is exact
    A, B = ar.doubled_midranks(X), ar.doubled_midranks(R)
    assert A.max() <= 2 * m and B.max() <= 2 * m
    sab = np.rint(A.astype(np.float64) @ B.astype(np.float64).T).astype(np.int64)
    spot = np.unique(np.concatenate([np.arange(0, n, 64), [n - 2]]))[-256:]
    assert len(spot) == 256 and spot[-1] == n - 1 and np.array_equal(sab[spot], ar.integers(X[spot], R)[0])
    assert_integers(r, sab, (A * A).sum(axis=1), (B * B).sum(axis=1))
    # scores: the last 64 cells of the full chunk (tiles of the second sweep: t >= 32 * cus means cell tile >= 32 * cus /
    # ts), the lone cell of the second chunk, every 257th cell
    first_second_sweep_cell = 16 * ((32 * cus) // ts + 1)
    assert first_second_sweep_cell <= annotate.MAX_CHUNK - 64
    cells = np.unique(np.concatenate([np.arange(annotate.MAX_CHUNK - 64, annotate.MAX_CHUNK), [n - 1], np.arange(0, n, 257)]))
    want, first = ar.scores(X[cells], R, labels, 3)
    print("grid cap: cus", cus, "S", S, "tiles", 1024 * ts, "cells scored on the CPU", len(cells),
          "bit-identical", int((r["scores"][cells] == want).sum()), "of", want.size)
    assert np.array_equal(r["scores"][cells], want)
    assert np.array_equal(r["first_labels"], np.argmax(r["scores"], axis=1))


# ---- 2. the quantile -------------------------------------------------------------------------------------------------------

def test_quantile_label_sizes_and_equal_rho():
    """label sizes 1 .. 12, 16, 256, 257, 513: the candidate loop strides (more than 256 samples per label), the
    interpolation at every small size; duplicated rows inside labels (equal rho, ties broken by index); cells that are the
    reverse of a sample (negative rho)"""
    sizes = list(range(1, 13)) + [16, 256, 257, 513]
    rng = np.random.default_rng(513)
    S, m, n, L = sum(sizes), 40, 24, len(sizes)
    labels = interleaved(rng, sizes)
    base = rows(rng, 1, m, zeros=0.1)[0]
    R = np.where(rng.random((S, m)) < 0.35, rows(rng, S, m, zeros=0.1), base).astype(np.float32)
    for l in (4, 9, 12, 13, 14, 15):                               # duplicated rows: a fifth of the label copies one sample
        s = np.flatnonzero(labels == l)
        R[s[1::5]] = R[s[0]]
    X = np.where(rng.random((n, m)) < 0.35, rows(rng, n, m), base).astype(np.float32)
    X[:6] = -R[rng.choice(S, 6, replace=False)]                    # anti-correlated with the reference
    want, first = ar.scores(X, R, labels, L)
    assert (want[:6] < 0).all() and (want[6:] > 0).any()
    r = annotate.score_pass(X, R, labels=labels)
    assert_integers(r, *ar.integers(X, R))
    print("quantile: scores bit-identical:", int((r["scores"] == want).sum()), "of", want.size,
          "max abs diff", np.abs(r["scores"] - want).max())
    assert np.array_equal(r["scores"], want)
    assert np.array_equal(r["first_labels"], np.argmax(r["scores"], axis=1))


# ---- 3. limits -------------------------------------------------------------------------------------------------------------

def test_sample_and_label_caps():
    S, L, m, n = annotate.MAX_SAMPLES, annotate.MAX_LABELS, 33, 5
    rng = np.random.default_rng(4096)
    labels = interleaved(rng, [1] * (L - 1) + [S - (L - 1)])
    X, R = rows(rng, n, m), rows(rng, S, m, zeros=0.1)
    want, first = ar.scores(X, R, labels, L)
    r = annotate.score_pass(X, R, labels=labels)
    assert_integers(r, *ar.integers(X, R))
    assert np.array_equal(r["scores"], want)
    assert np.array_equal(r["first_labels"], np.argmax(r["scores"], axis=1))
    with pytest.raises(_lib.MiSaError, match="S must be in"):
        annotate.score_pass(np.zeros((1, 4), np.float32), np.ones((S + 1, 4), np.float32))


# ---- 4. fine-tuning --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ec.NAMES)
def test_fine_tuning_edge_cases(name):
    c = ec.case(name)
    e = c.expect
    R = ec.full_reference(c)
    r = annotate.score_pass(c.X, R, labels=c.ids, masks=c.masks, fine_tune=True)
    print(name, "S", c.S, "m", c.m, "G' sizes", c.gsizes, "iterations", np.bincount(r["iterations"]),
          "bit-identical scores", int((r["scores"] == e["scores"]).sum()), "of", e["scores"].size,
          "tuned_best", int((r["tuned_best"] == e["tuned_best"]).sum()), "of", c.n,
          "largest differences", np.abs(r["scores"] - e["scores"]).max(), np.abs(r["tuned_best"] - e["tuned_best"]).max())
    for key in KEYS:
        assert np.array_equal(r[key], e[key]), key
    again = annotate.score_pass(c.X, R, labels=c.ids, masks=c.masks, fine_tune=True)
    for key in ("sab", "sa2", "sb2") + KEYS:
        assert np.array_equal(r[key], again[key]), key


# ---- 5. one handle, several chunks ------------------------------------------------------------------------------------------

def test_handle_reuse():
    c = ec.case("ref_zeros")
    rng = np.random.default_rng(129)
    big = c.X[rng.integers(0, c.n, 129)]
    small = c.X[[3, 59, 0, 17, 44, 8, 30]]
    with annotate.Annotator(c.R, c.ids, c.L, c.masks) as ann:
        s1 = ann.score(big)
        t1 = ann.fine_tune()
        assert t1["labels"].shape == (129,)
        s2 = ann.score(small)
        t2 = ann.fine_tune()
        t3 = ann.fine_tune()
    with annotate.Annotator(c.R, c.ids, c.L, c.masks) as fresh:
        f2 = fresh.score(small)
        ft = fresh.fine_tune()
    for key in ("scores", "first_labels"):
        assert np.array_equal(s2[key], f2[key]), key
    for key in ("labels", "tuned_best", "tuned_next", "iterations"):
        assert t2[key].shape == (7,)
        assert np.array_equal(t2[key], ft[key]), key
        assert np.array_equal(t3[key], t2[key]), key
    assert np.array_equal(t2["labels"], c.expect["labels"][[3, 59, 0, 17, 44, 8, 30]])


# ---- 6. a refused score call leaves no resident chunk ------------------------------------------------------------------------

def refusals(m):
    bad = np.ones((3, m), dtype=np.float32)
    bad[1, m // 2] = np.nan
    return {"nan": (bad, "not finite"), "over_chunk": (np.ones((annotate.MAX_CHUNK + 1, m), dtype=np.float32), "exceed a chunk")}


@pytest.mark.parametrize("kind", ["nan", "over_chunk"])
def test_refused_score_leaves_no_resident_chunk(kind):
    MI_ESTATE = annotate.MI_ESTATE
    c = ec.case("flat_on_g")
    bad, text = refusals(c.m)[kind]
    lib = _lib.load()
    f32p, f64p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    # the C entry first, with outputs sized for the EARLIER chunk: whatever the library did, it could not overrun them
    with annotate.Annotator(c.R, c.ids, c.L, c.masks) as ann:
        ann.score(c.X)
        rc = lib.mi_annot_score(ann._h, bad.ctypes.data_as(f32p), bad.shape[0], None, None, None, None, None, None)
        assert rc < 0 and text in lib.mi_last_error().decode()
        labels, iters = np.full(c.n, -7, dtype=np.int32), np.full(c.n, -7, dtype=np.int32)
        best, nxt = np.full(c.n, -7.0), np.full(c.n, -7.0)
        rc = lib.mi_annot_fine_tune(ann._h, labels.ctypes.data_as(i32p), best.ctypes.data_as(f64p), nxt.ctypes.data_as(f64p),
                                    iters.ctypes.data_as(i32p), None)
        assert rc == MI_ESTATE and "has not run" in lib.mi_last_error().decode()
        assert (labels == -7).all() and (iters == -7).all() and (best == -7.0).all() and (nxt == -7.0).all()
        # ... and a good chunk afterwards is resident again
        ann.score(c.X[:5])
        assert np.array_equal(ann.fine_tune()["labels"], c.expect["labels"][:5])
    # the same sequence through the Python handle
    with annotate.Annotator(c.R, c.ids, c.L, c.masks) as ann:
        ann.score(c.X)
        with pytest.raises(_lib.MiSaError, match=text):
            ann.score(bad)
        assert ann.n_c == 0
        with pytest.raises(_lib.MiSaError, match="has not run") as ei:
            ann.fine_tune()
        assert ei.value.code == MI_ESTATE
        ann.score(c.X[:5])
        assert np.array_equal(ann.fine_tune()["labels"], c.expect["labels"][:5])
