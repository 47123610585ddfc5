"""Cell-type annotation on the GPU (include/mi_annot.h, csrc/annot_kernels.hip) against the CPU restatement of
tests/annot_reference.py.  The sums of rank products are exact integers and are compared with ``np.array_equal`` at the digit
carry (m = 64), the wavefront and MFMA-k edges, the cap m = 8191, the tile edges of the cross pass, across chunks and on
special rows; the scores bit for bit (measured identical on the MI355X: the integers are exact and rho and the quantile are
the same correctly rounded fp64 operations in the same order; the project's fp64 tolerance, 1e-9, was the starting point);
and the fine-tuning loop label for label, iteration count for iteration count, on EVERY cell of the planted cases
(tests/test_annot_host.py shows that no decision of theirs is closer than 1e-6), then ``single_r`` end to end, dense
against sparse."""
import numpy as np
import pytest
import scipy.sparse as sp

import annot_cases
import annot_reference as ar
from markers_reference import tie_block_vectors
from scrna_seq_qannealing_clustering_amd import _lib, annotate, metrics

pytestmark = pytest.mark.gpu


def rows(rng, r, m, zeros=0.5):
    """log-normalised-looking rows: a share of zeros, small counts (ties) through log1p"""
    x = np.log1p(rng.integers(1, 6, (r, m)) * rng.choice([0.5, 1.0, 2.0], (r, 1)))
    x[rng.random((r, m)) < zeros] = 0.0
    return x.astype(np.float32)


def check_integers(X, R, **kw):
    sab, sa2, sb2 = ar.integers(X, R)
    r = annotate.score_pass(X, R, **kw)
    assert r["sab"].shape == sab.shape and r["sab"].dtype == np.int64
    assert np.array_equal(r["sa2"], sa2), "sum a^2"
    assert np.array_equal(r["sb2"], sb2), "sum b^2"
    assert np.array_equal(r["sab"], sab), "sum a b"
    return r


# ---- 1. exact integers -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 127, 128, 129])
def test_integers_gene_edges(m):
    rng = np.random.default_rng(m)
    X, R = rows(rng, 17, m), rows(rng, 17, m, zeros=0.1)
    X[0], R[0] = np.arange(m, 0, -1), np.arange(1, m + 1)           # all distinct: the largest ranks, digit carries from m = 64
    check_integers(X, R)


@pytest.mark.parametrize("S", [1, 2, 17])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 129])
def test_integers_cell_and_sample_edges(n, S):
    rng = np.random.default_rng(100 * n + S)
    check_integers(rows(rng, n, 65), rows(rng, S, 65, zeros=0.1))


def test_integers_at_the_gene_cap():
    m = annotate.MAX_GENES
    rng = np.random.default_rng(8191)
    X, R = rows(rng, 17, m), rows(rng, 2, m, zeros=0.05)
    perm = rng.permutation(m).astype(np.float32) + 1.0              # all distinct, the same order in the cell and the sample
    X[0], R[0] = perm, perm * 0.5
    X[1] = -perm                                                    # ... and the reverse order
    r = check_integers(X, R)
    big = 4 * m * (m + 1) * (2 * m + 1) // 6                        # sum (2 i)^2 in Python integers: the largest sum a b
    assert int(r["sab"][0, 0]) == big == int(r["sa2"][0]) == int(r["sb2"][0])
    assert int(r["sab"][1, 0]) == sum(2 * i * 2 * (m + 1 - i) for i in range(1, m + 1))


def test_chunks_equal_the_unsplit_run():
    rng = np.random.default_rng(5)
    X, R = rows(rng, 129, 65), rows(rng, 17, 65, zeros=0.1)
    labels = rng.permutation(np.arange(17) % 3)
    whole = check_integers(X, R, labels=labels)
    split = annotate.score_pass(X, R, labels=labels, chunk=65)
    for key in ("sab", "sa2", "sb2", "scores", "first_labels"):
        assert np.array_equal(whole[key], split[key]), key


def special_rows(rng, m=300):
    rws = {
        "all_zero": np.zeros(m),
        "no_zeros": rng.uniform(0.5, 3.0, m),
        "one_tie_group": np.full(m, 1.25),
        "all_distinct": rng.permutation(m) + 1.0,
        "counts_0_3": rng.integers(0, 4, m).astype(float),
        "negatives": rng.standard_normal(m),
        "both_zeros": np.where(rng.random(m) < 0.2, 1.5, np.where(rng.random(m) < 0.5, -0.0, 0.0)),
    }
    rws["both_zeros"][:4] = [-0.0, 0.0, -2.0, 2.0]
    for k in (255, 256, 257):
        c = np.zeros(m)
        c[rng.permutation(m)[:k]] = rng.uniform(0.1, 2.0, k)
        rws["nonzeros_%d" % k] = c
    return list(rws), np.stack(list(rws.values())).astype(np.float32)


def test_special_rows():
    rng = np.random.default_rng(2)
    names, X = special_rows(rng)
    z = X[names.index("both_zeros")]
    assert np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()
    assert [int((X[names.index("nonzeros_%d" % k)] != 0).sum()) for k in (255, 256, 257)] == [255, 256, 257]
    R = np.concatenate([X[::-1], rows(rng, 3, X.shape[1])])         # every special row meets every special row
    r = check_integers(X, R)
    m = X.shape[1]
    flat = m * (m + 1) ** 2                                         # every rank m + 1 (doubled): the all-zero and one-tie rows
    assert int(r["sa2"][names.index("all_zero")]) == flat == int(r["sa2"][names.index("one_tie_group")])
    # rho = 0 on the zero-variance rows, cell or sample
    for i in (names.index("all_zero"), names.index("one_tie_group")):
        assert not r["scores"][i].any()
    one = annotate.score_pass(X, X[[names.index("all_zero")]])
    assert not one["scores"].any()


def test_tie_blocks_at_both_ends():
    """rows whose tie runs touch sorted position 0 and the last one, cross position 256 and outgrow a workgroup
    (markers_reference.tie_block_vectors): as cells and, reversed, as samples; then as the samples of two labels whose
    pair markers are all the genes, so that the fine-tuning loop ranks every one of them again over G' = all genes"""
    rng = np.random.default_rng(18)                                  # (a seed at which every cell enters the loop: asserted below)
    X = tie_block_vectors(rng)[0]
    m = X.shape[1]
    check_integers(X, np.ascontiguousarray(X[::-1]))
    R, ids = tie_block_vectors(rng)[0], np.array([0, 1, 0], dtype=np.int32)      # the same blocks, other positions
    pairs = {(0, 1): np.arange(m), (1, 0): np.arange(m)}
    trace = []
    e = ar.annotate(X, R, ids, 2, pairs, trace=trace)
    assert sorted(t[0] for t in trace) == [0, 1, 2] and all(t[1:] == ((0, 1), m) for t in trace) and e["margin"].min() > 1e-6
    r = annotate.score_pass(X, R, labels=ids, masks=annotate.pair_masks(pairs, np.arange(m), 2), fine_tune=True)
    for key in ("scores", "first_labels", "iterations", "labels", "tuned_best", "tuned_next"):
        assert np.array_equal(r[key], e[key]), key


def test_limits_are_refused():
    with pytest.raises(_lib.MiSaError, match="m must be in"):
        annotate.score_pass(np.zeros((1, 8192), np.float32), np.zeros((1, 8192), np.float32))
    with pytest.raises(_lib.MiSaError, match="L must be in"):
        annotate.score_pass(np.zeros((1, 4), np.float32), np.ones((65, 4), np.float32), labels=np.arange(65))
    with pytest.raises(_lib.MiSaError, match="not finite"):
        annotate.score_pass(np.full((1, 4), np.nan, np.float32), np.ones((1, 4), np.float32))
    with pytest.raises(ValueError, match="chunk"):
        annotate.score_pass(np.zeros((1, 4), np.float32), np.ones((1, 4), np.float32), chunk=annotate.MAX_CHUNK + 1)


# ---- 2. scores -------------------------------------------------------------------------------------------------------------

def test_scores_and_quantile_sizes():
    """labels with 1, 2, 5 and 6 samples, interleaved in the caller's order; a constant sample and an all-zero cell"""
    rng = np.random.default_rng(7)
    labels = rng.permutation(np.repeat([0, 1, 2, 3], [1, 2, 5, 6]))
    X, R = rows(rng, 40, 100), rows(rng, 14, 100, zeros=0.1)
    X[3] = 0.0
    R[int(np.flatnonzero(labels == 2)[0])] = 2.0
    want, first = ar.scores(X, R, labels, 4)
    r = annotate.score_pass(X, R, labels=labels)
    print("scores bit-identical:", int((r["scores"] == want).sum()), "of", want.size, "max abs diff", np.abs(r["scores"] - want).max())
    assert np.array_equal(r["scores"], want)
    assert not r["scores"][3].any()
    assert np.array_equal(r["first_labels"], np.argmax(r["scores"], axis=1))      # lowest label id on ties (cell 3: all 0 -> 0)
    top = np.sort(want, axis=1)
    clear = top[:, -1] - top[:, -2] > 1e-6
    assert clear.sum() > 30 and np.array_equal(r["first_labels"][clear], first[clear])


# ---- 3. fine-tuning --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["L2", "L6", "L64"])
def test_fine_tuning_matches_the_restatement_on_every_cell(name):
    c = annot_cases.case(name)
    e = c.expect
    r = annotate.score_pass(c.XM, c.RM, labels=c.ref.label_ids, masks=c.masks, fine_tune=True)
    print(name, "iterations", np.bincount(r["iterations"]), "bit-identical tuned_best:", int((r["tuned_best"] == e["tuned_best"]).sum()),
          "of", c.n, "scores:", int((r["scores"] == e["scores"]).sum()), "of", e["scores"].size)
    assert np.array_equal(r["scores"], e["scores"])
    assert np.array_equal(r["first_labels"], e["first_labels"])
    assert np.array_equal(r["iterations"], e["iterations"])
    assert np.array_equal(r["labels"], e["labels"])
    assert np.array_equal(r["tuned_best"], e["tuned_best"])
    assert np.array_equal(r["tuned_next"], e["tuned_next"])
    counts = np.bincount(r["iterations"], minlength=3)
    if name == "L2":
        # the smallest loop: `use` is one label (no iteration), or both and then a stop after one iteration
        assert counts[0] > 0 and counts[1] > 0 and counts[2:].sum() == 0
        kept_both = (r["iterations"] == 1) & (r["tuned_best"] - r["tuned_next"] <= annotate.TUNE_THRESH)
        assert kept_both.any()                                      # a `use` that never shrinks stops after one iteration
    if name == "L6":
        assert counts[0] > 0 and counts[1] > 0 and counts[2:].sum() > 0
    # two calls on the same input return identical bits
    again = annotate.score_pass(c.XM, c.RM, labels=c.ref.label_ids, masks=c.masks, fine_tune=True)
    for key in ("sab", "scores", "first_labels", "labels", "tuned_best", "tuned_next", "iterations"):
        assert np.array_equal(r[key], again[key]), key


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------

def test_single_r_end_to_end_dense_and_sparse():
    c = annot_cases.case("L6")
    e = c.expect
    assert set(c.gene_names) != set(c.ref_gene_names) and len(c.test_idx) < c.g       # partial overlap, another order
    assert [c.gene_names[j] for j in c.test_idx] != [c.ref_gene_names[j] for j in sorted(c.ref_idx)]
    dense = annotate.single_r(c.X, c.gene_names, c.ref)
    sparse = annotate.single_r(sp.csr_matrix(c.X), c.gene_names, c.ref, chunk=128)     # three chunks
    for key in ("labels", "first_labels", "pruned_labels", "label_ids", "scores", "tuned_best", "tuned_next", "iterations",
                "delta"):
        assert np.array_equal(dense[key], sparse[key]), key
    assert dense["marker_genes"] == sparse["marker_genes"] == [c.gene_names[j] for j in c.test_idx[c.M]]
    values = np.array(c.ref.label_values, dtype=object)
    assert np.array_equal(dense["label_ids"], e["labels"])
    assert list(dense["labels"]) == list(values[e["labels"]])
    assert list(dense["first_labels"]) == list(values[e["first_labels"]])
    want_pruned = values[e["labels"]]
    want_pruned[e["pruned"]] = None
    assert list(dense["pruned_labels"]) == list(want_pruned) and e["pruned"].any()
    truth = values[c.truth]
    accuracy = np.mean(dense["labels"] == truth)
    assert accuracy >= np.mean(values[e["labels"]] == truth) and accuracy > 0.8
    ari = metrics.adjusted_rand_index(dense["label_ids"], c.truth)
    assert 0.5 < ari <= 1.0
    plain = annotate.single_r(c.X, c.gene_names, c.ref, fine_tune=False, prune=False)
    assert list(plain["labels"]) == list(dense["first_labels"]) == list(plain["pruned_labels"])
    assert not plain["iterations"].any() and np.array_equal(plain["scores"], dense["scores"])
