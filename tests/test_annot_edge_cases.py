"""The edge cases of tests/annot_edge_cases.py are what they claim (no GPU): shown on the CPU restatement alone.  Every
reference holds zeros of both signs, negatives and ties; the G' sizes met in the loop are the ones named; the iteration
histograms have the entries the device test relies on; and in the margin-checked cases every threshold test and argmax of
EVERY cell is decided by more than 1e-6 (the condition of tests/test_annot_host.py), so tests/test_gpu_annot_edges.py can
compare labels and iteration counts exactly.  The engineered exact ties (no markers, a duplicated label, |G'| <= 2, cells
that are flat on G') are exempt from the margin: there the tie and its lowest-id outcome are asserted directly."""
import numpy as np
import pytest

import annot_edge_cases as ec
import annot_reference as ar
from scrna_seq_qannealing_clustering_amd import annotate


@pytest.mark.parametrize("name", ec.NAMES)
def test_data_rules(name):
    c = ec.case(name)
    R, X = c.R, c.X                                                  # (the distinct rows where the case tiles them: test_cap)
    assert R.shape == ((c.S if c.row_of is None else c.row_of.max() + 1), c.m) and R.dtype == np.float32 and X.dtype == np.float32
    zero = R == 0
    share = zero.mean()
    print(name, "S", c.S, "m", c.m, "n", c.n, "zeros %.3f of them negative %.3f, negatives %.3f, levels %d"
          % (share, (zero & np.signbit(R)).sum() / zero.sum(), (R < 0).mean(), len(np.unique(R))))
    assert 0.07 < share < 0.18                                       # about a tenth: the zero block of every sample is non-empty
    assert zero.any(axis=1).all()
    assert (zero & np.signbit(R)).any() and (zero & ~np.signbit(R)).any()
    assert 0.01 < (R < 0).mean() < 0.06
    assert len(np.unique(R)) <= 16                                   # a handful of levels: tie groups everywhere
    assert (X == 0).mean() > 0.05 and len(np.unique(X)) < 40
    # interleaved: the labels are not grouped in the caller's order
    assert sorted(set(c.ids.tolist())) == list(range(c.L))
    assert (np.diff(c.ids) != 0).sum() >= c.L
    # the masks are the lists
    for (a, b), genes in c.pairs.items():
        row = c.masks[a * c.L + b]
        got = np.flatnonzero((row[:, None] >> np.arange(32, dtype=np.uint32)) & 1)
        assert np.array_equal(got, np.sort(genes)), (a, b)


@pytest.mark.parametrize("name", ec.MARGIN_CHECKED)
def test_every_decision_is_clear_of_rounding(name):
    c = ec.case(name)
    e = c.expect
    print(name, "iterations", np.bincount(e["iterations"]), "G' sizes", c.gsizes, "smallest margin %.3g" % e["margin"].min())
    assert e["margin"].shape == (c.n,) and e["margin"].min() > 1e-6


def test_ref_zeros():
    c = ec.case("ref_zeros")
    e = c.expect
    assert (c.L, c.m, c.n) == (6, 700, 60) and np.bincount(c.ids).tolist() == [1, 2, 3, 4, 5, 6]
    counts = np.bincount(e["iterations"])
    assert counts[0] > 0 and counts[1] > 0 and counts[2:].sum() > 0
    assert c.gsizes == [10, 14, 45, 55]
    # a smaller G' follows a larger one in the same workgroup: use drops from three or more labels to two
    shrinks = [i for i in range(c.n)
               if any(len(a) >= 3 and len(b) == 2 for a, b in zip(ec.uses_of(c, i), ec.uses_of(c, i)[1:]))]
    assert shrinks
    sizes = {i: [g for j, _, g in c.trace if j == i] for i in shrinks}
    print("cells whose use drops from 3+ labels to 2, with their G' sizes:", sizes)
    assert any(a > b for s in sizes.values() for a, b in zip(s, s[1:]))               # stale gidx / ar entries would show


def test_big_labels():
    c = ec.case("big_labels")
    e = c.expect
    assert np.bincount(c.ids).tolist() == [3, 70, 300] and (c.m, c.n) == (130, 12)
    assert c.gsizes == [10]
    tuned = e["iterations"] >= 1
    assert tuned.sum() >= 4 and all(set(u) == {1, 2} for i in np.flatnonzero(tuned) for u in ec.uses_of(c, i))
    assert len(c.copies) == 40 and (c.ids[c.copies] == 2).all() and (c.R[c.copies] == c.R[c.copies[0]]).all()
    # the run of 40 equal rho covers the order statistics lo = 239 and lo + 1 = 240 of label 2, for some cell
    sab, sa2, sb2 = ar.integers(c.X, c.R)
    big = np.flatnonzero(c.ids == 2)
    covered = 0
    for i in range(c.n):
        rho = np.array([ar.rho(c.m, sab[i, s], sa2[i], sb2[s]) for s in big])
        tie = ar.rho(c.m, sab[i, c.copies[0]], sa2[i], sb2[c.copies[0]])
        below, upto = int((rho < tie).sum()), int((rho <= tie).sum())
        assert upto - below >= 40
        covered += below <= 239 and upto >= 241
    print("cells whose label-2 quantile lies inside the tie run:", covered, "of", c.n)
    assert covered >= 1


@pytest.mark.parametrize("k", ec.G_SIZES)
def test_g_sizes(k):
    c = ec.case("g_%d" % k)
    e = c.expect
    assert (c.L, c.m) == (2, 1100) and c.gsizes == [k]
    G = np.unique(np.concatenate([c.pairs[(0, 1)], c.pairs[(1, 0)]]))
    assert len(G) == k and np.array_equal(G, c.genes)
    assert len(np.intersect1d(c.pairs[(0, 1)], c.pairs[(1, 0)])) >= 1 or k == 1          # the lists overlap
    if k >= 63:
        assert {0, 31, 32, c.m - 1} <= set(G.tolist())
        assert len(set((G >> 5).tolist())) >= min(k // 2, 30)                            # bits in many mask words
    assert (e["iterations"] == 1).all()                               # both labels in use at step 3, for every cell
    if k <= 2:
        # rho is exactly -1, 0 or 1, so scores tie exactly; the tie goes to the lower id
        sab, sa2, sb2 = ar.integers(c.X[:, G], c.R[:, G])
        assert {ar.rho(k, sab[i, s], sa2[i], sb2[s]) for i in range(c.n) for s in range(c.S)} <= {-1.0, 0.0, 1.0}
        tie = e["tuned_best"] == e["tuned_next"]
        assert tie.any() and (e["labels"][tie] == 0).all()
        assert (ec.step3_margin(e["scores"]) > 1e-6).all()            # step 3, on all 1100 genes, is clear
    if k == 1:
        assert tie.all() and not e["tuned_best"].any()


def test_no_markers():
    c = ec.case("no_markers")
    e = c.expect
    assert len(c.pairs[(0, 1)]) == 0 and len(c.pairs[(1, 0)]) == 0 and len(c.pairs[(0, 2)]) > 0 and len(c.pairs[(2, 1)]) > 0
    assert not c.masks[[1, 3]].any() and c.masks[[2, 5, 6, 7]].any(axis=1).all()
    assert c.gsizes == [0]                                            # label 2 is never in use together with a twin
    twins = np.flatnonzero(e["iterations"] >= 1)
    assert len(twins) >= 4 and all(ec.uses_of(c, i) == [(0, 1)] for i in twins)
    assert (e["iterations"][twins] == 1).all() and (e["labels"][twins] == 0).all()
    assert not e["tuned_best"][twins].any() and not e["tuned_next"][twins].any()
    assert (e["first_labels"][twins] == 1).any()                      # the tie-break changes a label: step 3 had chosen label 1
    assert (e["labels"] == 2).any() and (e["iterations"] == 0).any()
    assert (ec.step3_margin(e["scores"]) > 1e-6).all()


def test_duplicate_label():
    c = ec.case("duplicate_label")
    e = c.expect
    assert np.array_equal(c.R[c.ids == 2], c.R[c.ids == 1]) and len(c.pairs[(1, 2)]) > 0 and len(c.pairs[(2, 1)]) > 0
    assert np.array_equal(e["scores"][:, 1], e["scores"][:, 2])
    both = np.flatnonzero([ec.uses_of(c, i) == [(1, 2)] for i in range(c.n)])
    assert len(both) >= 4 and c.gsizes == [70]
    assert (e["iterations"][both] == 1).all() and (e["labels"][both] == 1).all() and (e["first_labels"][both] == 1).all()
    assert np.array_equal(e["tuned_best"][both], e["tuned_next"][both]) and e["tuned_best"][both].all()
    assert not ((e["tuned_best"] - e["tuned_next"]) < 0.0).any()      # the `< 0` rule of the pruning does not fire on a tie
    _, pruned = annotate.prune_scores(e["scores"], e["labels"], e["tuned_best"], e["tuned_next"])
    _, plain = annotate.prune_scores(e["scores"], e["labels"])
    assert np.array_equal(pruned, plain)
    # the decisions that are not the engineered tie are clear: label 0 against the pair, at step 3
    s = e["scores"]
    assert (np.abs(s[:, 0] - s[:, 1]) > 1e-6).all() and (np.abs(np.abs(s[:, 0] - s[:, 1]) - ar.TUNE_THRESH) > 1e-6).all()
    assert (e["iterations"] == 0).any() and (e["labels"] == 0).any()


def test_flat_on_g():
    c = ec.case("flat_on_g")
    e = c.expect
    G = c.G
    assert c.gsizes == [100] and np.array_equal(np.unique(np.concatenate(list(c.pairs.values()))), G)
    flat = np.zeros(c.n, dtype=bool)
    flat[c.flat] = True
    assert (c.X[flat][:, G] == 0).all() and (c.X[flat] != 0).any(axis=1).all()
    z = c.X[flat][:, G]
    assert np.signbit(z).any() and not np.signbit(z).all()
    for s in c.const_samples:
        assert len(np.unique(c.R[s, G])) == 1 and c.R[s, G[0]] != 0
    for s in c.zero_samples:
        assert (c.R[s, G] == 0).all() and np.signbit(c.R[s, G]).any() and not np.signbit(c.R[s, G]).all()
    assert sorted(c.ids[c.const_samples].tolist()) == [0, 1] == sorted(c.ids[c.zero_samples].tolist())
    # the flat cells: both labels in use, one pass, every rho 0, the lower id
    assert (e["iterations"][flat] == 1).all() and (e["labels"][flat] == 0).all()
    assert not e["tuned_best"][flat].any() and not e["tuned_next"][flat].any()
    assert (ec.step3_margin(e["scores"])[flat] > 1e-6).all()
    # the others: the flat samples give rho = 0 among non-zero ones, and every decision is clear
    assert (e["iterations"][~flat] == 1).sum() >= 4 and e["tuned_best"][~flat].all()
    assert e["margin"][~flat].min() > 1e-6
    B = ar.doubled_midranks(c.R[:, G])
    for s in c.const_samples + c.zero_samples:
        assert len(G) * int((B[s] * B[s]).sum()) == (len(G) * (len(G) + 1)) ** 2          # db == 0


@pytest.mark.parametrize("name", sorted(ec.CAP_VARIANTS))
def test_cap(name):
    c = ec.case(name)
    e = c.expect
    genes = ec.CAP_VARIANTS[name]
    assert (c.m, c.S, c.L, c.n) == (annotate.MAX_GENES, annotate.MAX_SAMPLES, 3, 6) == (8191, 4096, 3, 6)
    assert np.bincount(c.ids).tolist() == [3, 3, 4090]
    assert c.gsizes == [genes] and len(np.unique(np.concatenate([c.pairs[(0, 1)], c.pairs[(1, 0)]]))) == genes
    assert c.genes[0] == 0 and c.genes[-1] == c.m - 1
    assert len(set((c.genes >> 5).tolist())) == (c.m + 31) // 32      # every mask word has a bit
    assert (e["iterations"] == 1).all() and all(ec.uses_of(c, i) == [(0, 1)] for i in range(c.n))
    assert sorted(set(e["labels"].tolist())) == [0, 1]
    # label 2 is never near the threshold
    assert (e["scores"][:, 2] < e["scores"].max(axis=1) - 2 * ar.TUNE_THRESH).all()
    # the tiling: the reference is the 11 distinct rows indexed, and the indexed integers are the integers of the rows themselves
    full = ec.full_reference(c)
    assert c.R.shape == (11, c.m) and full.shape == (c.S, c.m) and full.flags.c_contiguous
    assert len(set(c.row_of[c.ids == 2].tolist())) == 5 and sorted(c.row_of[c.ids != 2].tolist()) == list(range(6))
    rows = np.concatenate([np.flatnonzero(c.ids != 2), np.arange(1000, 1012)])
    sab, sa2, sb2 = ar.integers(c.X, c.R)
    fab, fa2, fb2 = ar.integers(c.X, full[rows])
    assert np.array_equal(fab, sab[:, c.row_of[rows]]) and np.array_equal(fb2, sb2[c.row_of[rows]]) and np.array_equal(fa2, sa2)
