"""The host steps of the annotation chain (annotate.py; no GPU): the number of markers per pair, the classic markers against a
brute-force loop, the quantile, the pruning rule, the gene intersection, the argument checks of the C entry points (made
before any device work), and the margin condition that lets tests/test_gpu_annot.py compare the labels of every cell."""
import ctypes as C

import numpy as np
import pytest

import annot_cases
import annot_reference as ar
from scrna_seq_qannealing_clustering_amd import _lib, annotate


def test_de_n_values():
    assert [annotate.default_de_n(L) for L in (2, 10, 29, 64)] == [333, 130, 70, 44]


def test_module_is_exported():
    import scrna_seq_qannealing_clustering_amd as pkg
    assert pkg.annotate is annotate and "annotate" in pkg.__all__


# ---- classic markers -------------------------------------------------------------------------------------------------------

def toy_reference():
    """3 labels, 2-3 samples each, 12 genes; medians chosen so that pairs tie, vanish and run short of de_n"""
    med = np.array([
        # g0   g1   g2   g3   g4   g5   g6   g7   g8   g9  g10  g11
        [3.0, 3.0, 1.0, 2.0, 2.0, 0.0, 5.0, 1.0, 1.0, 4.0, 0.5, 2.0],      # label "a"
        [1.0, 1.0, 1.0, 2.0, 3.0, 0.0, 5.0, 1.0, 2.0, 1.0, 0.5, 2.0],      # label "b": a - b ties at g0 = g1 = 2, then g9 = 3
        [1.0, 1.0, 1.0, 2.0, 3.0, 0.0, 5.0, 1.0, 2.0, 1.0, 0.5, 2.5],      # label "c": b - c is never positive
    ])
    labels = ["a", "b", "a", "c", "b", "c", "a"]
    ids = np.array([0, 1, 0, 2, 1, 2, 0])
    rng = np.random.default_rng(3)
    R = med[ids].copy()
    # label a has three samples: the outer two move apart symmetrically, the median stays; b and c have two: +-d keeps the mean
    R[0] += 0.25
    R[6] -= 0.25
    for l in (1, 2):
        s = np.flatnonzero(ids == l)
        d = rng.integers(0, 8, 12) / 64.0                  # exact in binary: (m + d + m - d) / 2 == m
        R[s[0]] += d
        R[s[1]] -= d
    return R, labels, ids, med


def test_classic_markers_against_brute_force():
    R, labels, ids, med = toy_reference()
    assert np.array_equal(annotate.label_medians(R, ids, 3), med)
    for de_n in (1, 2, 3, 12):
        pairs, M = annotate.classic_markers(R, labels, de_n=de_n)
        bp, bM = ar.brute_markers(R, ids, 3, de_n)
        assert sorted(pairs) == sorted(bp)
        for ab in bp:
            assert list(pairs[ab]) == bp[ab], (de_n, ab)
        assert list(M) == bM
    pairs, M = annotate.classic_markers(R, labels, de_n=2)
    assert list(pairs[(0, 1)]) == [9, 0]                    # 3.0 first, then the tie g0 = g1 = 2.0 goes to the lower index
    assert list(pairs[(1, 2)]) == []                        # no positive difference: nothing is kept
    assert list(pairs[(2, 1)]) == [11]                      # fewer positive genes than de_n
    assert list(pairs[(1, 0)]) == [4, 8]
    pairs, M = annotate.classic_markers(R, labels, de_n=12)
    assert list(pairs[(0, 1)]) == [9, 0, 1] and list(pairs[(0, 2)]) == [9, 0, 1]
    assert list(M) == [0, 1, 4, 8, 9, 11]


def test_pair_masks_are_the_lists():
    R, labels, ids, _ = toy_reference()
    pairs, M = annotate.classic_markers(R, labels, de_n=12)
    masks = annotate.pair_masks(pairs, M, 3)
    assert masks.shape == (9, 1) and masks.dtype == np.uint32
    for (a, b), genes in pairs.items():
        assert sorted(int(M[j]) for j in range(len(M)) if (int(masks[a * 3 + b, 0]) >> j) & 1) == sorted(genes)
    assert not masks[[0, 4, 8]].any()
    wide = annotate.pair_masks({(0, 1): np.arange(0, 70, 3), (1, 0): np.array([69])}, np.arange(70), 2)
    assert wide.shape == (4, 3) and int(wide[2, 2]) == 1 << 5 and int(wide[1, 0]) & 0b1001001 == 0b1001001


# ---- the quantile ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", [1, 2, 5, 6])
def test_quantile(s):
    rng = np.random.default_rng(s)
    c = rng.standard_normal(s)
    srt = np.sort(c)
    want = {1: lambda: srt[0], 2: lambda: srt[0] + 0.8 * (srt[1] - srt[0]),
            5: lambda: srt[3] + (0.8 * 4 - 3) * (srt[4] - srt[3]), 6: lambda: srt[4]}[s]()
    assert annotate.quantile(c) == want == ar.quantile(c)
    if s == 6:
        assert 0.8 * 5 == 4.0                               # lands on an order statistic: no interpolation term
    assert abs(annotate.quantile(c) - np.quantile(c, 0.8)) < 1e-12


# ---- pruning ---------------------------------------------------------------------------------------------------------------

def test_prune_scores():
    # label 0: nine cells with deltas near 0.5 and one outlier far below; label 1: one cell only
    delta0 = np.array([0.50, 0.52, 0.48, 0.51, 0.49, 0.50, 0.53, 0.47, 0.50, 0.05])
    scores = np.zeros((11, 3))
    scores[:10, 0] = delta0                                 # max - median = delta (the median of (d, 0, 0) is 0)
    scores[10] = [0.1, 0.3, 0.2]
    labels = np.array([0] * 10 + [1])
    delta, pruned = annotate.prune_scores(scores, labels)
    assert np.allclose(delta[:10], delta0, rtol=0, atol=0) and delta[10] == 0.3 - 0.2
    med = np.median(delta0)
    mad = np.median(np.abs(delta0 - med))
    assert delta0[9] < med - 3 * 1.4826 * mad < delta0[:9].min()
    assert list(np.flatnonzero(pruned)) == [9]              # the outlier; the single cell of label 1 has MAD 0, delta == median
    # a negative tuned margin prunes too
    best, nxt = np.ones(11), np.zeros(11)
    nxt[3] = 1.5
    _, pruned = annotate.prune_scores(scores, labels, best, nxt)
    assert list(np.flatnonzero(pruned)) == [3, 9]
    rd, rp = ar.prune(scores, labels, best, nxt)
    assert np.array_equal(rd, delta) and np.array_equal(rp, pruned)


# ---- gene intersection -----------------------------------------------------------------------------------------------------

def test_common_genes_order_and_duplicates():
    t, r = annotate.common_genes(["A", "B", "C", "D", "E"], ["E", "X", "C", "A"])
    assert list(t) == [0, 2, 4] and list(r) == [3, 2, 0]    # the test list's order
    with pytest.raises(ValueError, match="duplicate gene name 'B' in the test"):
        annotate.common_genes(["A", "B", "B"], ["A"])
    with pytest.raises(ValueError, match="duplicate gene name 'A' in the reference"):
        annotate.common_genes(["A", "B"], ["A", "A"])
    t, r = annotate.common_genes(["A"], ["B"])
    assert len(t) == 0 and len(r) == 0


def test_label_ids_follow_first_appearance():
    ids, values = annotate.encode_labels(["T", "B", "T", ("NK", 1), "B"])
    assert list(ids) == [0, 1, 0, 2, 1] and values == ["T", "B", ("NK", 1)]


def test_reference_markers_depend_on_the_common_genes():
    R, labels, ids, med = toy_reference()
    ref = annotate.Reference(R.astype(np.float32), ["g%d" % j for j in range(12)], labels, de_n=1)
    pairs, M = ref.markers
    assert list(pairs[(0, 1)]) == [9]
    sub = np.array([0, 1, 2, 3])                            # without g9 the pair's best gene is g0
    pairs, M = ref.markers_on(sub)
    assert list(pairs[(0, 1)]) == [0] and list(M) == [0]
    with pytest.raises(ValueError, match="NaN or an infinity"):
        annotate.Reference(np.full((2, 2), np.nan), ["a", "b"], [0, 1])


# ---- argument checks of the C entry points: refused before any device work ----------------------------------------------

def create_rc(S, m, L, labels=None, R=None, masks=None):
    lib = _lib.load()
    R = np.ones((S, m), dtype=np.float32) if R is None else np.ascontiguousarray(R, dtype=np.float32)
    labels = (np.arange(S) % max(L, 1)).astype(np.int32) if labels is None else np.asarray(labels, dtype=np.int32)
    masks = np.zeros((max(L, 1) ** 2, (m + 31) // 32), dtype=np.uint32) if masks is None else masks
    h = C.c_void_p()
    rc = lib.mi_annot_create(R.ctypes.data_as(C.POINTER(C.c_float)), S, m, labels.ctypes.data_as(C.POINTER(C.c_int32)), L,
                             masks.ctypes.data_as(C.POINTER(C.c_uint32)), 0, C.byref(h), None)
    assert not h.value
    return rc, lib.mi_last_error().decode()


def test_limits_are_refused_before_device_work():
    EINVAL, EUNSUPPORTED = -1, None
    with pytest.raises(_lib.MiSaError) as ei:
        _lib.check(create_rc(2, 8192, 1)[0])
    EUNSUPPORTED = ei.value.code
    assert EUNSUPPORTED != EINVAL and "m must be in [1, 8191]" in ei.value.message
    for S, m, L, text in [(2, 0, 1, "m must be"), (70, 4, 65, "L must be"), (2, 4, 0, "L must be"), (2, 4, 3, "S must be"),
                          (4097, 1, 1, "S must be")]:
        rc, msg = create_rc(S, m, L)
        assert rc == EUNSUPPORTED and text in msg, (S, m, L, msg)
    rc, msg = create_rc(3, 4, 2, labels=[0, 0, 0])
    assert rc == EINVAL and "label 1 has no samples" in msg
    rc, msg = create_rc(3, 4, 2, labels=[0, 2, 1])
    assert rc == EINVAL and "not in [0, 2)" in msg
    for bad in (np.nan, np.inf, -np.inf):
        R = np.ones((3, 4), dtype=np.float32)
        R[1, 2] = bad
        rc, msg = create_rc(3, 4, 2, R=R)
        assert rc == EINVAL and "R[1, 2] is not finite" in msg
    masks = np.zeros((4, 1), dtype=np.uint32)
    masks[1, 0] = 1 << 4
    rc, msg = create_rc(3, 4, 2, masks=masks)
    assert rc == EINVAL and "past m" in msg
    lib = _lib.load()
    assert lib.mi_annot_score(None, None, 1, None, None, None, None, None, None) == EINVAL
    assert lib.mi_annot_fine_tune(None, None, None, None, None, None) == EINVAL
    assert lib.mi_annot_destroy(None) == 0


# ---- the margin condition --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(annot_cases.SPECS))
def test_planted_cases_keep_every_decision_clear_of_rounding(name):
    """Every threshold test and argmax of the restatement is decided by more than 1e-6, ten orders of magnitude above the
    rounding of an fp64 score: the device must reproduce the labels and iteration counts of ALL cells."""
    c = annot_cases.case(name)
    e = c.expect
    print(name, "m", len(c.M), "iterations", np.bincount(e["iterations"]), "smallest margin %.3g" % e["margin"].min())
    assert e["margin"].min() > 1e-6
    assert 1 <= len(c.M) <= annotate.MAX_GENES
    counts = np.bincount(e["iterations"], minlength=3)
    if name == "L2":
        assert counts[0] > 0 and counts[1] > 0 and counts[2:].sum() == 0
        both = (e["iterations"] == 1) & (e["tuned_best"] - e["tuned_next"] <= 0.05)
        assert both.any()                                   # `use` never shrank: one iteration, then the stop
    if name == "L6":
        assert counts[0] > 0 and counts[1] > 0 and counts[2:].sum() > 0
    if name == "L64":
        assert c.ref.de_n == 44 and c.RM.shape[0] == 64
