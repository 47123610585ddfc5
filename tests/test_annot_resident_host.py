"""Annotation on the resident expression handle, off the GPU: the three exports and their NULL refusals, the argument checks
of ``single_r`` that come before any device work, and the numpy restatement of the cluster means
(tests/annot_resident_reference.py) against a plain Python loop and against an order-blind sum."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import annot_resident_reference as rr
from scrna_seq_qannealing_clustering_amd import _lib, annotate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mi_annot_score_matrix", "mi_annot_score_clusters", "mi_annot_fetch_chunk")
EINVAL = -1


def test_new_names_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "mi_annot.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS
        assert re.search(r"^int %s\s*\(" % name, header, flags=re.M), name
        getattr(lib, name)
    assert len(_lib._SIG["mi_annot_score_matrix"][1]) == 12 and len(_lib._SIG["mi_annot_score_clusters"][1]) == 13


def test_null_handles_are_refused_before_device_work():
    lib = _lib.load()
    ms = (C.c_float * 4)(7.0, 7.0, 7.0, 7.0)
    assert lib.mi_annot_score_matrix(None, None, 1, None, 0, 1, None, None, None, None, None, ms) == EINVAL
    assert list(ms) == [0.0] * 4                                 # zeroed first, as every entry does
    assert lib.mi_annot_score_clusters(None, None, 1, None, None, 1, None, None, None, None, None, None, None) == EINVAL
    assert lib.mi_annot_fetch_chunk(None, None) == EINVAL
    assert "NULL" in lib.mi_last_error().decode()


def test_single_r_checks_which_and_clusters_before_any_device_work():
    c = rr.planted()
    with pytest.raises(ValueError, match="which must be"):
        annotate.single_r(c.X, c.gene_names, c.ref, which="data")
    with pytest.raises(ValueError, match="which must be"):
        annotate.single_r(c.X, c.gene_names, c.ref, which=1)
    for bad in (np.zeros(c.n - 1, dtype=int), list(range(c.n + 1)), []):
        with pytest.raises(ValueError, match="one label per cell"):
            annotate.single_r(c.X, c.gene_names, c.ref, clusters=bad)


def test_restatement_equals_a_plain_loop():
    rng = np.random.default_rng(2)
    X = rng.random((9, 5)).astype(np.float32)
    cols, of = [4, 0, 2], [1, 0, 1, 1, 2, 0, 1, 2, 1]
    means, sizes = rr.cluster_means_reference(X, cols, of)
    assert means.dtype == np.float32 and sizes.tolist() == [2, 5, 2]
    for c in range(3):
        for s, j in enumerate(cols):
            total, count = 0.0, 0                                # Python floats are fp64
            for i in range(9):
                if of[i] == c:
                    total += float(X[i, j])
                    count += 1
            assert means[c, s] == np.float32(total / count)


def test_the_order_of_the_sum_shows_in_the_bits_of_the_gpu_cases():
    """the GPU test compares bit for bit: on the counts of the "base" matrix at K = 2 an order-blind (pairwise) sum differs
    from the sequential one in the mean of the last gene (ORDER_SENSITIVE), so a reduction in another order fails there"""
    X = rr.matrix("base")
    lab = rr.interleaved_labels(2)
    assert (lab[:4] == 0).all() and (lab == 0).sum() == 64
    for m in (65, 130):
        cols = rr.marker_cols(X.shape[1], m, seed=2)
        s = int(np.flatnonzero(cols == X.shape[1] - 1)[0])
        seq, pair = rr.cluster_means_reference(X, cols, lab)[0], rr.pairwise_means(X, cols, lab)
        print("m", m, "sequential", float(seq[0, s]).hex(), "pairwise", float(pair[0, s]).hex())
        assert seq[0, s] == np.float32(2.0 ** -6) and pair[0, s] == np.nextafter(np.float32(2.0 ** -6), np.float32(1.0))
        assert (seq != pair).sum() == 1


def test_shared_cases_have_the_edges_the_gpu_tests_name():
    for name in ("base", "wide"):
        X = rr.matrix(name)
        assert X.shape[0] == rr.N and not X[rr.ZERO_CELL].any() and not X[:, rr.EMPTY_GENE].any()
        assert 0.05 < (X != 0).mean() < 0.2
        for m in rr.M_LIST:
            cols = rr.marker_cols(X.shape[1], m)
            assert len(set(cols.tolist())) == m == len(cols)
            if m >= 3:
                assert {0, X.shape[1] - 1, rr.EMPTY_GENE} <= set(cols.tolist())
        A = rr.csr_with_stored_zeros(X, rr.marker_cols(X.shape[1], 130))
        assert (A.data == 0).sum() == 18 and A[:, rr.EMPTY_GENE].nnz == 0
    assert (rr.matrix("wide")[rr.LONG_ROW] != 0).sum() == 700
    for K in rr.K_LIST:
        lab = rr.interleaved_labels(K)
        assert sorted(set(lab.tolist())) == list(range(K)) and (K == 1 or (np.diff(lab) < 0).any())
    assert (rr.interleaved_labels(65) == 64).sum() == 1
