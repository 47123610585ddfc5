"""SCTransform's corrected counts off the GPU: the scalar function every kernel form calls (``mi_sct::corrected_count``,
csrc/mi_sct_math.h), compiled as a host program under the sanitizers, against the numpy restatement
(tests/sct_correct_reference.py); the restatement on the inputs of the GPU tests (no entry next to a half-integer, zeros that
become counts and counts that become zeros); ``metrics.pack_expression`` of a sparse matrix; and the three new exports."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import prep_reference as ref
import prep_regress_cases as rc
import sct_correct_reference as cr
from scrna_seq_qannealing_clustering_amd import _lib, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def grid():
    """(x, mu, alpha, mu_r) rows: every combination of a few counts, means over seven decades, dispersions from Poisson to
    heavy, and reference means a drawn factor away from mu (a round factor would put whole families of values on the
    half-integers); then the edges: equal means (the identity), a vanishing and a huge mean"""
    rng = np.random.default_rng(42)
    xs = np.array([0.0, 1.0, 2.0, 3.0, 7.0, 40.0, 1000.0, 50000.0])
    mus = 10.0 ** np.linspace(-4.0, 3.0, 15) * rng.uniform(0.9, 1.1, 15)
    alphas = np.array([0.0, 0.013, 0.4, 1.0, 9.7])
    factors = 10.0 ** rng.uniform(-1.0, 1.0, 6)
    x, mu, al, f = (a.ravel() for a in np.meshgrid(xs, mus, alphas, factors, indexing="ij"))
    rows = np.column_stack([x, mu, al, mu * f])
    edges = np.array([[5.0, 0.3, 0.2, 0.3], [0.0, 2.5, 0.0, 2.5], [12.0, 1e-300, 0.5, 1e-300], [3.0, 1e300, 0.0, 1e299],
                      [0.0, 1e-12, 1.0, 30.0], [1.0, 1e-12, 1.0, 30.0]])
    return np.vstack([rows, edges])


def test_scalar_function_as_a_host_program_equals_the_restatement(tmp_path):
    exe = str(tmp_path / "sct_correct_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "host", "sct_correct_main.cpp")], check=True)
    G = grid()
    text = "".join("%s %s %s %s\n" % tuple(float(v).hex() for v in row) for row in G)
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    out = [line.split() for line in run.stdout.splitlines()]
    assert len(out) == len(G)
    got = np.array([float.fromhex(t[0]) for t in out])
    finite = np.array([t[1] == "1" for t in out])
    with np.errstate(all="ignore"):
        v = cr.value(G[:, 0], G[:, 1], G[:, 2], G[:, 3])
    assert np.array_equal(finite, np.isfinite(v))
    assert finite[:-6].all() and finite.sum() >= len(G) - 2       # (1e300 squared overflows: the flag's case)
    ok = finite
    assert not cr.near_half(v[ok]).any()                         # the grid leaves no entry out of the comparison
    assert np.array_equal(got[ok], cr.count_of(v[ok]))
    assert (got[ok] == 0).any() and (got[ok] > 0).any() and not np.signbit(got).any()
    # the identity: equal means give the count back
    same = G[:, 1] == G[:, 3]
    assert same.sum() >= 3 and np.array_equal(got[same & ok], G[same & ok, 0])


SHAPES = [(n, 65) for n in (2, 255, 256, 257, 1027)] + [(257, g) for g in (1, 63, 64, 150)]


@pytest.mark.parametrize("n,g", SHAPES)
def test_restatement_on_the_gpu_tests_inputs_has_no_entry_next_to_a_half_integer(n, g):
    X, lu, b0, b1, alpha, lu_ref = cr.inputs(n, g)
    genes = cr.listed_genes(g)
    v = cr.values(X[:, genes], b0[genes], b1[genes], alpha[genes], lu, lu_ref)
    frac = np.abs(np.abs(v - np.floor(v)) - 0.5)
    c = cr.count_of(v)
    grew, fell = int(((X[:, genes] == 0) & (c != 0)).sum()), int(((X[:, genes] != 0) & (c == 0)).sum())
    print("(%d, %d): nearest to a half-integer %.3g; zero -> count %d, count -> zero %d, density %.2f -> %.2f"
          % (n, g, frac.min(), grew, fell, (X[:, genes] != 0).mean(), (c != 0).mean()))
    assert np.isfinite(v).all() and not cr.near_half(v).any()
    if n >= 255 and g >= 63:
        assert grew > 0 and fell > 0


def test_restatement_identity_at_the_reference_depth():
    X, _, b0, b1, alpha, _ = cr.inputs(257, 65)
    c, near = cr.corrected(X, np.arange(65), b0, b1, alpha, np.full(257, 3.25), 3.25)
    assert not near.any() and np.array_equal(c, X)


@pytest.mark.parametrize("g", [1, 63, 64, 65, 130])
def test_pack_expression_of_a_sparse_matrix_equals_that_of_the_dense_one(g):
    X = ref.sparse_counts(np.random.default_rng(g), 70, g)
    X, A = rc.csr_with_stored_zeros_and_empty_row(X, np.random.default_rng(g + 1))
    assert (A.data == 0).any() and (np.diff(A.indptr) == 0).any()
    want = metrics.pack_expression(X)
    for M in (A, A.tocsc(), A.tocoo(), sp.csr_matrix(X)):
        got = metrics.pack_expression(M)
        assert got.dtype == np.uint64 and got.shape == (70, (g + 63) // 64) and np.array_equal(got, want)
    empty = metrics.pack_expression(sp.csr_matrix((5, g), dtype=np.float32))
    assert empty.shape == (5, (g + 63) // 64) and not empty.any()


def test_new_symbols_are_exported_with_the_documented_signatures():
    hdr = open(os.path.join(ROOT, "include", "mi_prep.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    for decl in ("int mi_prep_sct_correct(mi_prep_matrix *m, const int32_t *genes, int gp, const double *b0, const double *b1, "
                 "const double *alpha, const double *log_umi, double log_umi_ref, mi_prep_matrix **out, float *out_kernel_ms);",
                 "int mi_prep_fetch_counts(mi_prep_matrix *m, float *out);",
                 "int mi_prep_fetch_csr(mi_prep_matrix *m, int64_t *indptr, int32_t *indices, float *data);"):
        assert decl in flat, decl
    lib = C.CDLL(_lib.LIB_PATH)
    f32p, f64p, i32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    want = {"mi_prep_sct_correct": [C.c_void_p, i32p, C.c_int, f64p, f64p, f64p, f64p, C.c_double, C.POINTER(C.c_void_p), f32p],
            "mi_prep_fetch_counts": [C.c_void_p, f32p],
            "mi_prep_fetch_csr": [C.c_void_p, i64p, i32p, f32p]}
    sig = _lib._signatures()
    for name, args in want.items():
        assert hasattr(lib, name) and name in _lib.EXPORTS
        assert sig[name][0] is C.c_int and sig[name][1] == args
    # the NULL checks come before any device work
    h = C.c_void_p()
    loaded = _lib.load()
    assert loaded.mi_prep_sct_correct(None, None, 1, None, None, None, None, 3.0, C.byref(h), None) == -1 and not h.value
    assert loaded.mi_prep_fetch_counts(None, None) == -1 and loaded.mi_prep_fetch_csr(None, None, None, None) == -1
