"""ctypes binding of ``libmi_sa.so`` (include/mi_sa.h).  There is no CPU fallback: if the HIP library
is missing or cannot be loaded this module raises, loudly."""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MI_SA_LIB selects another build of the same library (e.g. the -DMI_K2_PROFILE development build)
LIB_PATH = os.environ.get("MI_SA_LIB") or os.path.join(_HERE, "libmi_sa.so")

MI_OK = 0
KIND_DENSE, KIND_CSR_RANK1, KIND_POTTS_CSR = 1, 2, 3

_lock = threading.Lock()
_lib = None


class MiSaError(RuntimeError):
    """Error reported by the native engine (negative MI_E* code + message)."""

    def __init__(self, code, message):
        super().__init__("libmi_sa error %d: %s" % (code, message))
        self.code = code
        self.message = message


def _signatures():
    """Every export of libmi_sa.so, written once: name -> (result type, argument types)."""
    u8p, u16p, u32p, u64p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint16, C.c_uint32, C.c_uint64))
    i32p, i64p, f32p, f64p = (C.POINTER(t) for t in (C.c_int32, C.c_int64, C.c_float, C.c_double))
    ip = C.POINTER(C.c_int)              # the headers' ``int *`` (out scalars); ``int32_t *`` (arrays) is i32p
    vp, pp = C.c_void_p, C.POINTER(C.c_void_p)
    sig = {
        "mi_last_error": (C.c_char_p, []),
        "mi_abi_version": (C.c_int, []),
        "mi_device_count": (C.c_int, [ip]),
        "mi_device_info": (C.c_int, [C.c_int, C.c_char_p, C.c_int, ip, u64p]),
        "mi_sa_problem_create_dense_f32": (C.c_int, [f32p, C.c_int, C.c_double, C.c_int, pp]),
        "mi_sa_problem_create_csr_rank1_f32": (C.c_int, [i32p, i32p, f32p, f32p, C.c_float, C.c_int,
                                                         C.c_double, C.c_int, pp]),
        "mi_sa_problem_create_potts_csr_f32": (C.c_int, [i32p, i32p, f32p, C.c_float, C.c_int,
                                                         C.c_int, C.c_double, C.c_int, pp]),
        "mi_sa_problem_destroy": (C.c_int, [vp]),
        "mi_sa_problem_info": (C.c_int, [vp, ip, ip, ip, ip]),
        "mi_sa_set_option": (C.c_int, [vp, C.c_char_p, C.c_long]),
        "mi_sa_plan_slot_order": (C.c_int, [i32p, i32p, C.c_int, C.c_int, i64p]),
        "mi_sa_plan_anneal": (C.c_int, [C.c_int, i32p, i32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int,
                                        C.c_int, C.c_char_p, C.c_int, ip]),
        "mi_sa_plan_dense": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_int,
                                       ip, u64p]),
        "mi_sa_problem_set_absent": (C.c_int, [vp, u8p]),
        "mi_sa_problem_set_pair_weights": (C.c_int, [vp, i32p]),
        "mi_sa_problem_set_node_weights": (C.c_int, [vp, i32p, f32p,
                                                     f64p]),
        "mi_sa_problem_set_node_weight_groups": (C.c_int, [vp, C.c_int, f32p,
                                                           f64p, f64p]),
        "mi_sa_problem_set_merge_moves": (C.c_int, [vp, C.c_int, C.c_int, f64p]),
        "mi_sa_plan_slot_layout": (C.c_int, [i32p, i32p, C.c_int, C.c_int, C.c_int, i64p, ip, ip]),
        "mi_sa_problem_set_energy_model_f64": (C.c_int, [vp, f64p, f64p, C.c_double]),
        "mi_sa_debug_pace": (C.c_int, [vp, u32p, C.c_int]),
        "mi_sa_debug_stats": (C.c_int, [vp, u64p, C.c_int]),
        "mi_sa_anneal": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_int, f64p, C.c_uint64, vp, C.c_int]),
        "mi_sa_anneal_ex": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_int, f64p, C.c_uint64, vp, C.c_int,
                                      C.c_uint32, C.c_uint32]),
        "mi_sa_tempering_begin": (C.c_int, [vp, f64p, C.c_int, C.c_int, C.c_uint32, C.c_int]),
        "mi_sa_tempering_exchange": (C.c_int, [vp, C.c_uint32, C.c_uint64, f64p]),
        "mi_sa_tempering_exchange_dev": (C.c_int, [vp, C.c_uint32, C.c_uint64, vp]),
        "mi_sa_device_results": (C.c_int, [vp, pp, pp, ip]),
        "mi_sa_tempering_state": (C.c_int, [vp, i32p, u64p, u64p]),
        "mi_sa_sync": (C.c_int, [vp]),
        "mi_sa_last_kernel_ms": (C.c_int, [vp, f32p]),
        "mi_sa_last_launch_count": (C.c_int, [vp, ip]),
        "mi_sa_last_kernel_name": (C.c_int, [vp, C.c_char_p, C.c_int]),
        "mi_sa_last_adjacency_bytes_per_slot": (C.c_int, [vp, ip]),
        "mi_sa_fetch": (C.c_int, [vp, vp, f64p, u64p]),
        "mi_sa_best": (C.c_int, [vp, ip, f64p, u64p, vp]),
        "mi_multi_gpu_anneal": (C.c_int, [pp, C.c_int, C.c_int, C.c_uint32, C.c_int, f64p, C.c_uint64, C.c_int]),
        "mi_multi_gpu_best": (C.c_int, [pp, C.c_int, ip, u32p, f64p, vp]),
        "mi_multi_gpu_fetch": (C.c_int, [pp, C.c_int, vp, f64p, u64p]),
        "mi_sa_qubo_dense_f32": (C.c_int, [f32p, C.c_int, C.c_double, C.c_int, C.c_int, f64p,
                                           C.c_uint64, u8p, u8p, f64p, u64p, C.c_int]),
        "mi_energy_dense_f32": (C.c_int, [f32p, C.c_int, u8p, C.c_int, C.c_double, f64p, C.c_int]),
        "mi_energy_dense_f64": (C.c_int, [f64p, C.c_int, u8p, C.c_int, C.c_double, f64p, C.c_int]),
        "mi_energy_dense_f32_ex": (C.c_int, [f32p, C.c_int, u8p, C.c_int, C.c_double, f64p, C.c_int, C.c_int,
                                             f32p]),
        # include/mi_snn.h
        "mi_snn_build_f32": (C.c_int, [f32p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, pp]),
        "mi_snn_build_ex_f32": (C.c_int, [f32p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_uint32, C.c_double,
                                          C.c_int, C.c_int, pp]),
        "mi_snn_build_rounded_f32": (C.c_int, [f32p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_double,
                                               C.c_int, pp]),
        "mi_snn_fetch_codes": (C.c_int, [vp, u8p]),
        "mi_snn_info": (C.c_int, [vp, ip, ip, i64p, ip]),
        "mi_snn_fetch": (C.c_int, [vp, i32p, i64p, i32p, i32p]),
        "mi_snn_kernel_ms": (C.c_int, [vp, f32p, f32p, f32p]),
        "mi_snn_destroy": (C.c_int, [vp]),
        # include/mi_metrics.h
        "mi_jaccard_cluster_stats": (C.c_int, [u64p, C.c_int, C.c_int, i32p, C.c_int, C.c_int, f64p, f64p, f64p, f64p,
                                               f64p, f32p, f32p]),
        "mi_label_agreement_u16": (C.c_int, [u16p, C.c_int, u16p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_int, f64p, f64p, i64p, i32p, f32p]),
        "mi_sa_problem_label_agreement": (C.c_int, [vp, C.c_int, f64p, f64p, i64p, f32p]),
        "mi_coassociation_u16": (C.c_int, [u16p, C.c_int, C.c_int, C.c_int, C.c_int, u16p, C.c_int, i32p, i32p, C.c_int64,
                                           C.c_int, i64p, i64p, i32p, i32p, f32p]),
        "mi_sa_problem_coassociation": (C.c_int, [vp, C.c_int, u16p, C.c_int, i32p, i32p, C.c_int64, i64p,
                                                  i64p, i32p, i32p, f32p]),
        "mi_graph_components": (C.c_int, [i32p, i32p, C.c_int, u16p, u8p, C.c_int, C.c_int, C.c_uint32, i32p, i32p, f32p]),
        "mi_sa_problem_components": (C.c_int, [vp, i32p, i32p, f32p]),
        "mi_rank_sum_markers_f32": (C.c_int, [f32p, C.c_int, C.c_int, u16p, C.c_int, C.c_int, C.c_int, C.c_uint32,
                                              i64p, i32p, f64p, i64p, f32p]),
        # include/mi_prep.h
        "mi_prep_create_f32": (C.c_int, [f32p, C.c_int, C.c_int, C.c_int, pp]),
        "mi_prep_create_csr_f32": (C.c_int, [i64p, i32p, f32p, C.c_int, C.c_int, C.c_int, pp]),
        "mi_prep_destroy": (C.c_int, [vp]),
        "mi_prep_info": (C.c_int, [vp, ip, ip, i64p, ip, i64p]),
        "mi_prep_fetch_normalized_csr": (C.c_int, [vp, f32p]),
        "mi_prep_normalize": (C.c_int, [vp, C.c_double, f32p]),
        "mi_prep_fetch_normalized": (C.c_int, [vp, f32p]),
        "mi_prep_gene_stats": (C.c_int, [vp, C.c_int, f64p, f64p, i32p, f32p]),
        "mi_prep_clipped_variance": (C.c_int, [vp, f64p, f64p, C.c_double, f64p, f32p]),
        "mi_prep_select": (C.c_int, [vp, i32p, C.c_int, f64p, f64p, C.c_double, f32p]),
        "mi_prep_fetch_scaled": (C.c_int, [vp, f32p]),
        "mi_prep_cell_qc": (C.c_int, [vp, u8p, f64p, i32p, f64p, f32p]),
        "mi_prep_select_regressed": (C.c_int, [vp, i32p, C.c_int, f64p, C.c_int, C.c_double, f64p, f64p, f64p, u8p, f32p]),
        "mi_prep_gene_log1p_sum": (C.c_int, [vp, f64p, f32p]),
        "mi_prep_nb_fit": (C.c_int, [vp, i32p, C.c_int, i32p, C.c_int, f64p, f64p, f64p, f64p, f64p, f64p, f64p, i32p, u8p, u8p,
                                     f32p]),
        "mi_prep_sct_residual_moments": (C.c_int, [vp, i32p, C.c_int, f64p, f64p, f64p, f64p, C.c_double, f64p, f64p, f32p]),
        "mi_prep_sct_select": (C.c_int, [vp, i32p, C.c_int, f64p, f64p, f64p, f64p, C.c_double, f64p, C.c_int, f64p, f64p, f64p,
                                         u8p, f32p]),
        "mi_prep_sct_correct": (C.c_int, [vp, i32p, C.c_int, f64p, f64p, f64p, f64p, C.c_double, pp, f32p]),
        "mi_prep_fetch_counts": (C.c_int, [vp, f32p]),
        "mi_prep_fetch_csr": (C.c_int, [vp, i64p, i32p, f32p]),
        "mi_prep_gram": (C.c_int, [vp, f64p, f32p]),
        "mi_prep_project": (C.c_int, [vp, f32p, C.c_int, f32p, f32p]),
        "mi_prep_rank_sum_markers": (C.c_int, [vp, C.c_int, u16p, C.c_int, C.c_int, C.c_uint32, i64p, i32p, f64p,
                                               i64p, f32p]),
        # include/mi_umap.h
        "mi_umap_knn_f32": (C.c_int, [f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, pp, f32p]),
        "mi_umap_destroy": (C.c_int, [vp]),
        "mi_umap_fetch_knn": (C.c_int, [vp, i32p, f32p]),
        "mi_umap_smooth": (C.c_int, [vp, f32p]),
        "mi_umap_fetch_smooth": (C.c_int, [vp, f64p, f64p]),
        "mi_umap_union": (C.c_int, [vp, f32p]),
        "mi_umap_info": (C.c_int, [vp, ip, ip, i64p, ip, f32p]),
        "mi_umap_fetch_graph": (C.c_int, [vp, i64p, i32p, f32p]),
        "mi_umap_layout_f32": (C.c_int, [C.c_int, C.c_int, i64p, i32p, f32p, f32p, C.c_float, C.c_float,
                                         C.c_float, C.c_int, C.c_int, C.c_uint64, C.c_int, f32p, f32p]),
        "mi_umap_query_knn_f32": (C.c_int, [f32p, C.c_int, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, pp, f32p]),
        "mi_umap_query_destroy": (C.c_int, [vp]),
        "mi_umap_query_fetch_knn": (C.c_int, [vp, i32p, f32p]),
        "mi_umap_query_smooth": (C.c_int, [vp, f32p]),
        "mi_umap_query_fetch_smooth": (C.c_int, [vp, f64p, f32p]),
        "mi_umap_query_vote": (C.c_int, [vp, i32p, C.c_int, C.c_int, i32p, f64p, f64p, f32p]),
        "mi_umap_query_init": (C.c_int, [vp, C.c_int, f32p, f32p, f32p]),
        "mi_umap_transform_layout_f32": (C.c_int, [C.c_int, C.c_int, i32p, f32p, C.c_int, C.c_int, f32p, f32p, C.c_float,
                                                   C.c_float, C.c_float, C.c_int, C.c_int, C.c_uint64, C.c_int64, C.c_int,
                                                   f32p, f32p]),
        # include/mi_anchors.h
        "mi_anchors_find_f32": (C.c_int, [f32p, C.c_int, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, pp, f32p]),
        "mi_anchors_destroy": (C.c_int, [vp]),
        "mi_anchors_info": (C.c_int, [vp, ip, ip, i64p, i64p, f32p]),
        "mi_anchors_fetch": (C.c_int, [vp, i32p, i32p, i32p, i32p, i32p, i32p]),
        "mi_anchors_set_scores": (C.c_int, [vp, f64p]),
        "mi_anchors_weights": (C.c_int, [vp, C.c_int, C.c_double, f32p]),
        "mi_anchors_fetch_weights": (C.c_int, [vp, i64p, i32p, f64p, i32p, f32p]),
        "mi_anchors_predict_labels": (C.c_int, [vp, i32p, C.c_int, i32p, f64p, f64p, f32p]),
        "mi_anchors_predict_features": (C.c_int, [vp, f32p, C.c_int, f32p, f32p]),
        # include/mi_tsne.h
        "mi_tsne_knn_f32": (C.c_int, [f32p, C.c_int, C.c_int, C.c_double, C.c_int, pp, f32p]),
        "mi_tsne_destroy": (C.c_int, [vp]),
        "mi_tsne_fetch_knn": (C.c_int, [vp, i32p, f32p]),
        "mi_tsne_calibrate": (C.c_int, [vp, f32p]),
        "mi_tsne_fetch_calibration": (C.c_int, [vp, f64p, f32p]),
        "mi_tsne_symmetrize": (C.c_int, [vp, f32p]),
        "mi_tsne_info": (C.c_int, [vp, ip, ip, i64p, ip]),
        "mi_tsne_fetch_graph": (C.c_int, [vp, i64p, i32p, f32p]),
        "mi_tsne_layout_f32": (C.c_int, [C.c_int, C.c_int, i64p, i32p, f32p, f32p, f32p, f32p, C.c_float, C.c_float, C.c_int,
                                         C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p, f32p,
                                         f64p, f32p]),
        "mi_tsne_kl_f32": (C.c_int, [C.c_int, C.c_int, i64p, i32p, f32p, f32p, C.c_int, f64p, f32p]),
        # include/mi_annot.h
        "mi_annot_create": (C.c_int, [f32p, C.c_int, C.c_int, i32p, C.c_int, u32p, C.c_int, pp, f32p]),
        "mi_annot_destroy": (C.c_int, [vp]),
        "mi_annot_score": (C.c_int, [vp, f32p, C.c_int, i64p, i64p, i64p, f64p,
                                     i32p, f32p]),
        "mi_annot_fine_tune": (C.c_int, [vp, i32p, f64p, f64p, i32p, f32p]),
        "mi_annot_score_matrix": (C.c_int, [vp, vp, C.c_int, i32p, C.c_int, C.c_int, i64p, i64p, i64p, f64p, i32p, f32p]),
        "mi_annot_score_clusters": (C.c_int, [vp, vp, C.c_int, i32p, i32p, C.c_int, i32p, i64p, i64p, i64p, f64p, i32p,
                                              f32p]),
        "mi_annot_fetch_chunk": (C.c_int, [vp, f32p]),
    }
    return sig


_SIG = _signatures()
EXPORTS = tuple(_SIG)


def _declare(lib):
    for name, (res, args) in _SIG.items():
        fn = getattr(lib, name)          # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args


def load():
    """Load (once) and return the ctypes library.  PyTorch, when importable, is imported first so
    that this process holds ONE HIP runtime: torch bundles its own ``libamdhip64.so`` with the same
    SONAME that libmi_sa.so needs, and whichever is mapped first serves both."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "MI355X engine not built: %s is missing.  Build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` or "
                "`make -C scrna_seq_qannealing_clustering_amd/csrc`.  There is no CPU fallback."
                % LIB_PATH)
        try:
            import torch  # noqa: F401  (maps torch's HIP runtime first; see docstring)
        except Exception:
            pass
        try:
            lib = C.CDLL(LIB_PATH, mode=getattr(os, "RTLD_NOW", 2))
        except OSError as exc:
            raise RuntimeError("cannot load %s: %s (no CPU fallback exists)" % (LIB_PATH, exc)) from exc
        _declare(lib)
        _lib = lib
        return _lib


def check(code):
    if code != MI_OK:
        msg = load().mi_last_error()
        raise MiSaError(code, msg.decode("utf-8", "replace") if msg else "")
    return code


# POINTER(T) -> (T, the numpy dtype an array handed to such a parameter must have; None where no array is taken)
_POINTEE = {t: (t._type_, None if t._type_ is C.c_void_p else np.dtype(t._type_))
            for _, types in _SIG.values() for t in types if isinstance(t, type) and issubclass(t, C._Pointer)}


def _marshal(name, i, want, a):
    """Argument ``i`` of export ``name`` as ctypes takes it for the declared type ``want``: checked, never converted."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        if want is C.c_void_p:
            dtype = a.dtype                                  # (states: uint8 or uint16; any dtype, its address)
        elif want in _POINTEE:
            dtype = _POINTEE[want][1]
        else:
            raise TypeError("%s: argument %d takes %s, not an array" % (name, i, want.__name__))
        if a.dtype != dtype or not a.flags.c_contiguous:
            raise TypeError("%s: argument %d needs a C-contiguous %s array (got %s%s)"
                            % (name, i, dtype, a.dtype, "" if a.flags.c_contiguous else ", not C-contiguous"))
        return a.ctypes.data_as(want)
    if want in _POINTEE and isinstance(a, _POINTEE[want][0]):
        return C.byref(a)                                    # an out scalar, or the c_void_p an out-handle lands in
    return a


def call(name, *args):
    """The one path from the package into the library: export ``name`` of ``_SIG`` with every argument passed by its
    declared type, the return code through :func:`check`.

    A ``POINTER(T)`` parameter takes a C-contiguous ndarray of dtype T (anything else is a ``TypeError`` naming the
    export, the zero-based position and both dtypes: a silent copy would lose an output) or a ctypes instance of T,
    which goes by reference.  A ``c_void_p`` parameter takes a C-contiguous ndarray of any dtype, an ``int`` (a device
    address such as a torch ``data_ptr()``) or a ``c_void_p`` handle.  ``None`` is NULL; everything else (Python
    scalars, bytes, ctypes arrays and string buffers, explicit ``c_uint32`` / ``c_uint64``) goes through as it is."""
    types = _SIG[name][1]
    if len(args) != len(types):
        raise TypeError("%s takes %d arguments (%d given)" % (name, len(types), len(args)))
    fn = getattr(load(), name)
    return check(fn(*[_marshal(name, i, t, a) for i, (t, a) in enumerate(zip(types, args))]))


def call_ms(name, *args) -> float:
    """:func:`call` for an export whose last parameter is ``float *out_kernel_ms``: ``args`` without it; returns the ms."""
    if _SIG[name][1][-1] != C.POINTER(C.c_float):
        raise TypeError("%s does not end in a float *out_kernel_ms" % name)
    ms = C.c_float(0.0)
    call(name, *args, ms)
    return float(ms.value)


class Handle:
    """Owner of one native handle: ``_h`` is the open ``c_void_p`` or None, ``_destroy`` names the export that frees it
    (a class attribute of the wrappers; ``Handle(h, "mi_x_destroy")`` owns a bare handle for a ``with`` block).
    A context manager; using it after :meth:`close` is a ``ValueError`` raised before any call into the library."""
    _destroy = None
    _h = None                                                # (an instance made by ``__new__`` alone is closed)

    def __init__(self, h, destroy):
        self._h, self._destroy = h, destroy

    def _handle(self):
        if self._h is None or not self._h.value:
            raise ValueError("the %s is closed" % type(self).__name__)
        return self._h

    def close(self):
        h, self._h = self._h, None
        if h is not None and h.value:
            getattr(load(), self._destroy)(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_count() -> int:
    n = C.c_int(0)
    rc = load().mi_device_count(C.byref(n))
    if rc != MI_OK:
        return 0
    return int(n.value)


def device_info(device: int = 0):
    name = C.create_string_buffer(256)
    cus = C.c_int(0)
    mem = C.c_uint64(0)
    call("mi_device_info", device, name, 256, cus, mem)
    return {"name": name.value.decode(), "compute_units": int(cus.value), "hbm_bytes": int(mem.value)}
