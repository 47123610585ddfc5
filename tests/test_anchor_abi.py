"""libmi_sa.so exports every name include/mi_anchors.h declares, and the Python binding declares each with the header's
parameter count (no compute: CPU box)."""
import ctypes
import os
import re

from scrna_seq_qannealing_clustering_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declarations():
    """name -> number of parameters, from the header with its comments removed"""
    src = open(os.path.join(ROOT, "include", "mi_anchors.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {name: len(args.split(",")) for name, args in re.findall(r"\b(mi_anchors_[a-z0-9_]+)\s*\(([^)]*)\)", src)}


def test_header_names_the_entry_points_of_the_issue():
    want = {"mi_anchors_find_f32", "mi_anchors_fetch", "mi_anchors_set_scores", "mi_anchors_weights", "mi_anchors_fetch_weights",
            "mi_anchors_predict_labels", "mi_anchors_predict_features", "mi_anchors_destroy", "mi_anchors_info"}
    assert set(declarations()) == want


def test_library_exports_and_binding_declares_every_name():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in declarations().items():
        assert hasattr(lib, name), "libmi_sa.so does not export %s" % name
        assert name in _lib.EXPORTS and len(_lib._SIG[name][1]) == nargs, name


def test_null_handle_is_refused_without_a_device():
    lib = _lib.load()
    assert lib.mi_anchors_info(None, None, None, None, None, None) == -1 and b"NULL" in lib.mi_last_error()
    assert lib.mi_anchors_destroy(None) == 0
    h = ctypes.c_void_p()
    assert lib.mi_anchors_find_f32(None, 4, None, 4, 2, 2, 2, 1, 0, ctypes.byref(h), None) == -1 and not h.value
