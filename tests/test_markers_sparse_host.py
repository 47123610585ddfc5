"""Marker genes on a resident ``ExpressionMatrix`` or a ``scipy.sparse`` matrix, the parts that need no GPU: the symbol
``mi_prep_rank_sum_markers`` is declared and exported, refuses a NULL handle before any device work, and the shape and
argument errors of the new branches of ``metrics.rank_sum_pass`` / ``metrics.find_all_markers`` and of
``ExpressionMatrix.rank_sum_pass`` are raised before any library call; csrc/mi_markers_plan.h (the launch plan from the
stored counts) runs in a stand-alone program under AddressSanitizer and UBSan (tests/host/markers_plan_main.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from scrna_seq_qannealing_clustering_amd import _lib, metrics, preprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def test_symbol_is_declared_and_exported():
    assert "mi_prep_rank_sum_markers" in _lib.EXPORTS
    lib = _lib.load()
    fn = lib.mi_prep_rank_sum_markers
    assert fn.restype is C.c_int and len(fn.argtypes) == 11
    assert hasattr(C.CDLL(_lib.LIB_PATH), "mi_prep_rank_sum_markers")
    hdr = open(os.path.join(ROOT, "include", "mi_prep.h")).read()
    assert re.search(r"\bint mi_prep_rank_sum_markers\(mi_prep_matrix \*m, int which,", hdr)
    val = lambda name: int(re.search(r"#define %s\s+(\d+)" % name, hdr).group(1))
    assert (val("MI_PREP_MARKERS_COUNTS"), val("MI_PREP_MARKERS_NORMALIZED")) == (0, 1)
    assert (val("MI_PREP_MARKERS_GATHER_INPLACE"), val("MI_PREP_MARKERS_GATHER_PERMUTE")) == (4, 8)


def test_null_handle_is_refused_without_a_device():
    lib = _lib.load()
    L = np.zeros(4, dtype=np.uint16)
    out = np.zeros(4, dtype=np.int64)
    ms = C.c_float(-1.0)
    rc = lib.mi_prep_rank_sum_markers(None, 0, L.ctypes.data_as(C.POINTER(C.c_uint16)), 1, 1, 0,
                                      out.ctypes.data_as(C.POINTER(C.c_int64)), None, None, None, C.byref(ms))
    assert rc == EINVAL and b"NULL" in lib.mi_last_error() and ms.value == 0.0


def test_plan_is_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "markers_plan_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "host", "markers_plan_main.cpp")],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok"), run.stdout + run.stderr


@pytest.fixture
def no_library(monkeypatch):
    """any load of the library from here on is a failure of the test"""
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", refuse)


def closed_handle(n=6, g=3, sparse=True):
    """an ExpressionMatrix as it is after close(): the shape, no native handle"""
    m = object.__new__(preprocess.ExpressionMatrix)
    m.n, m.g, m.sparse, m.normalized, m.timing, m._h, m._lib = n, g, sparse, False, {}, None, None
    return m


def test_sparse_matrix_errors_come_before_any_library_call(no_library):
    A = sp.csr_matrix(np.eye(6, 3, dtype=np.float32))
    lab = np.arange(6) % 2
    with pytest.raises(ValueError, match="L"):
        metrics.rank_sum_pass(A, np.zeros(7, dtype=int), 2)
    with pytest.raises(ValueError, match="L"):
        metrics.rank_sum_pass(A, np.zeros((2, 2, 3), dtype=int), 2)
    with pytest.raises(ValueError, match="which"):
        metrics.rank_sum_pass(A, lab, 2, which="normalized")
    with pytest.raises(ValueError, match="which"):
        metrics.find_all_markers(A, lab, which="scaled")
    with pytest.raises(ValueError, match="labels"):
        metrics.find_all_markers(A, np.zeros(5, dtype=int))
    with pytest.raises(ValueError, match="labels"):
        metrics.find_all_markers(A, np.zeros((2, 3, 6), dtype=int))
    with pytest.raises(ValueError, match="genes"):
        metrics.find_all_markers(A, lab, genes=["a", "b"])
    with pytest.raises(ValueError, match="distinct cluster ids"):
        metrics.find_all_markers(A, np.arange(6 * 13).reshape(13, 6))
    # which= has no meaning for a dense array, whose path is the old one
    with pytest.raises(TypeError):
        metrics.rank_sum_pass(np.ones((6, 3), dtype=np.float32), lab, 2, which="counts")
    with pytest.raises(TypeError):
        metrics.find_all_markers(np.ones((6, 3), dtype=np.float32), lab, which="counts")


def test_handle_errors_come_before_any_library_call(no_library):
    m = closed_handle()
    lab = np.arange(6) % 2
    with pytest.raises(ValueError, match="which"):
        m.rank_sum_pass(lab, 2, which="scaled")
    with pytest.raises(ValueError, match="gather"):
        m.rank_sum_pass(lab, 2, which="counts", gather="sorted")
    with pytest.raises(ValueError, match="L must be"):
        m.rank_sum_pass(np.zeros(5, dtype=int), 2, which="counts")
    with pytest.raises(ValueError, match="labels"):
        m.rank_sum_pass(lab - 1, 2, which="counts")
    with pytest.raises(ValueError, match="labels"):
        m.rank_sum_pass(lab + 65535, 2, which="counts")
    with pytest.raises(ValueError, match="labels"):
        m.rank_sum_pass(lab * 0.5, 2, which="counts")
    with pytest.raises(ValueError, match="closed"):
        m.rank_sum_pass(lab, 2, which="counts")
    with pytest.raises(ValueError, match="which"):
        metrics.rank_sum_pass(m, lab, 2, which="scaled")
    with pytest.raises(ValueError, match="closed"):
        metrics.rank_sum_pass(m, lab, 2)
    with pytest.raises(ValueError, match="closed"):
        metrics.find_all_markers(m, lab)


def test_metrics_imports_preprocess_lazily():
    top = [line for line in open(metrics.__file__).read().splitlines() if line.startswith(("import ", "from "))]
    assert top and not any("preprocess" in line for line in top), top
