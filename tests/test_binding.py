"""The binding layer (_lib.call / call_ms / Handle) and the signature table against the headers.  No GPU: the real library is
touched only up to its own argument validation, everything else runs against a recording stub."""
import ctypes as C
import gc
import os
import re

import numpy as np
import pytest

from scrna_seq_qannealing_clustering_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "scrna_seq_qannealing_clustering_amd")

# ---- 1. include/*.h against _SIG ---------------------------------------------------------------------------------------

SCALARS = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "double": C.c_double, "unsigned int": C.c_uint32,
           "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "uint16_t": C.c_uint16,
           "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
# device addresses, declared untyped on purpose: (export, position) -> what the header says
DEVICE_ADDRESSES = {("mi_sa_tempering_exchange_dev", 3): C.POINTER(C.c_double),
                    ("mi_sa_device_results", 2): C.POINTER(C.POINTER(C.c_double))}


def ctype_of(decl):
    """the ctypes type of a C type as the headers spell it (qualifiers dropped)"""
    stars = decl.count("*")
    base = " ".join(w for w in decl.replace("*", " ").split() if w != "const")
    if base == "void" and stars == 0:
        return None
    if base == "char" and stars == 1:
        return C.c_char_p
    if base == "void" or base.startswith("mi_"):              # opaque: a handle, or untyped memory
        assert 1 <= stars <= 2, decl
        return C.c_void_p if stars == 1 else C.POINTER(C.c_void_p)
    t = SCALARS[base]
    for _ in range(stars):
        t = C.POINTER(t)
    return t


def header_prototypes():
    """{export: (result type, [parameter types])} of every prototype in include/*.h"""
    protos = {}
    for hdr in sorted(os.listdir(os.path.join(ROOT, "include"))):
        src = open(os.path.join(ROOT, "include", hdr)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        src = re.sub(r"//[^\n]*", "", src)
        for res, name, params in re.findall(r"^([A-Za-z_][\w \t\*]*?)\b(mi_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src, flags=re.M):
            assert name not in protos, "%s is declared twice" % name
            params = " ".join(params.split())
            types = []
            if params != "void":
                for p in params.split(","):
                    m = re.match(r"^(.*?)(\w+)$", p.strip())      # the type, then the parameter's name
                    assert m and m.group(1).strip(), "%s: cannot parse parameter %r" % (name, p)
                    types.append(ctype_of(m.group(1)))
            protos[name] = (ctype_of(res), types)
    return protos


def test_sig_matches_the_headers():
    protos = header_prototypes()
    assert len(protos) == len(_lib.EXPORTS)                    # a regex that skips a prototype must not pass
    assert sorted(protos) == sorted(_lib.EXPORTS)
    differ = set()
    for name, (res, types) in protos.items():
        sres, stypes = _lib._SIG[name]
        assert sres == res, "%s: result %s, header %s" % (name, sres, res)
        assert len(stypes) == len(types), "%s: %d arguments, header %d" % (name, len(stypes), len(types))
        for i, (s, t) in enumerate(zip(stypes, types)):
            if s != t:
                differ.add((name, i))
                assert DEVICE_ADDRESSES.get((name, i)) == t, "%s argument %d: %s, header %s" % (name, i, s, t)
    assert differ == set(DEVICE_ADDRESSES)                     # an allowed difference that stops being one fails too
    assert _lib._SIG["mi_sa_tempering_exchange_dev"][1][3] is C.c_void_p
    assert _lib._SIG["mi_sa_device_results"][1][2] == C.POINTER(C.c_void_p)


# ---- 2. marshalling against a recording stub ----------------------------------------------------------------------------

class Recorder:
    """stands in for the loaded library: every export records its arguments and returns 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("mi_"):
            raise AttributeError(name)

        def export(*args):
            self.calls.append((name, args))
            return 0
        return export


@pytest.fixture
def stub(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(_lib, "_lib", rec)
    return rec


def address(p):
    return C.cast(p, C.c_void_p).value


def regressed_args(h=2, n=3, q=2):
    """a correct argument list of mi_prep_select_regressed: int32, float64 and uint8 pointers plus scalars"""
    return [C.c_void_p(0x1000), np.arange(h, dtype=np.int32), h, np.ones((n, q)), q, 10.0, np.empty((q, h)), np.empty(h),
            np.empty(h), np.empty(h, dtype=np.uint8), C.c_float(0.0)]


def test_call_passes_arrays_scalars_none_and_out_values(stub):
    args = regressed_args()
    args[7] = None
    assert _lib.call("mi_prep_select_regressed", *args) == 0
    (name, got), = stub.calls
    assert name == "mi_prep_select_regressed" and len(got) == 11
    assert got[0] is args[0]                                   # a handle goes as it is
    for i, t in ((1, C.c_int32), (3, C.c_double), (6, C.c_double), (8, C.c_double), (9, C.c_uint8)):
        assert isinstance(got[i], C.POINTER(t)) and address(got[i]) == args[i].ctypes.data
    assert got[2] == 2 and got[4] == 2 and got[5] == 10.0
    assert got[7] is None
    C.cast(got[10], C.POINTER(C.c_float))[0] = 2.5             # by reference: the caller's c_float
    assert args[10].value == 2.5


def test_call_ms_appends_the_out_scalar(stub, monkeypatch):
    def export(*args):
        C.cast(args[-1], C.POINTER(C.c_float))[0] = 1.25
        stub.calls.append(args)
        return 0
    monkeypatch.setattr(stub, "mi_prep_select_regressed", export, raising=False)
    ms = _lib.call_ms("mi_prep_select_regressed", *regressed_args()[:-1])
    assert type(ms) is float and ms == 1.25 and len(stub.calls[0]) == 11


def test_void_pointer_parameters(stub):
    st = np.zeros((2, 3), dtype=np.uint16)
    _lib.call("mi_sa_fetch", 0xABCD00, st, None, None)         # an int is a device address
    _lib.call("mi_sa_tempering_exchange_dev", C.c_void_p(1), C.c_uint32(0), C.c_uint64(0), 0x7F0000001000)
    out = C.c_void_p()
    _lib.call("mi_prep_create_f32", np.zeros((1, 1), dtype=np.float32), 1, 1, 0, out)
    fetch, exchange, create = (a for _, a in stub.calls)
    assert fetch[0] == 0xABCD00 and address(fetch[1]) == st.ctypes.data
    assert exchange[3] == 0x7F0000001000
    C.cast(create[4], C.POINTER(C.c_void_p))[0] = 0x55         # the out-handle goes by reference
    assert out.value == 0x55
    with pytest.raises(TypeError, match=r"mi_sa_fetch.*argument 1"):
        _lib.call("mi_sa_fetch", 1, np.zeros((4, 4), dtype=np.uint8)[:, ::2], None, None)


def test_other_values_pass_untouched(stub):
    handles = (C.c_void_p * 2)(1, 2)
    name = C.create_string_buffer(16)
    _lib.call("mi_multi_gpu_fetch", handles, 2, None, None, None)
    _lib.call("mi_sa_last_kernel_name", C.c_void_p(1), name, 16)
    _lib.call("mi_sa_set_option", C.c_void_p(1), b"key", 3)
    assert stub.calls[0][1][0] is handles and stub.calls[1][1][1] is name and stub.calls[2][1][1:] == (b"key", 3)


@pytest.mark.parametrize("position, bad, needs", [
    (10, np.empty(1, dtype=np.float64), "float32"),            # a float64 array for a float *
    (1, np.arange(2, dtype=np.int64), "int32"),                # an int64 array for an int32_t *
    (7, np.empty(4)[::2], "float64"),                          # a non-contiguous slice
    (3, np.asfortranarray(np.ones((3, 2))), "float64"),        # a Fortran-ordered 2-d array
    (9, np.zeros(2, dtype=bool), "uint8"),                     # a bool array is not a uint8 array
])
def test_call_refuses_a_wrong_array(stub, position, bad, needs):
    args = regressed_args()
    args[position] = bad
    with pytest.raises(TypeError, match=r"mi_prep_select_regressed.*argument %d\b.*%s" % (position, needs)) as ei:
        _lib.call("mi_prep_select_regressed", *args)
    assert str(bad.dtype) in str(ei.value)
    assert stub.calls == []


def test_call_refuses_a_wrong_argument_count(stub):
    with pytest.raises(TypeError, match="mi_prep_select_regressed takes 11"):
        _lib.call("mi_prep_select_regressed", *regressed_args()[:-1])
    with pytest.raises(TypeError, match="mi_prep_select_regressed takes 11"):
        _lib.call_ms("mi_prep_select_regressed", *regressed_args())
    assert stub.calls == []


def test_an_empty_array_of_the_right_dtype_passes(stub):
    args = regressed_args()
    args[1] = np.empty(0, dtype=np.int32)
    _lib.call("mi_prep_select_regressed", *args)
    assert len(stub.calls) == 1


# ---- 3. the real library, up to its own validation -------------------------------------------------------------------------

def test_call_raises_the_library_error():
    with pytest.raises(_lib.MiSaError) as ei:
        _lib.call("mi_sa_problem_create_dense_f32", None, 4, 0.0, 0, C.c_void_p())
    assert ei.value.code == -1 and "NULL" in ei.value.message


def test_call_ms_needs_a_trailing_float_pointer(stub):
    with pytest.raises(TypeError, match="mi_sa_sync"):
        _lib.call_ms("mi_sa_sync", C.c_void_p(1))
    with pytest.raises(TypeError, match="mi_umap_fetch_smooth"):
        _lib.call_ms("mi_umap_fetch_smooth", C.c_void_p(1), np.empty(1))
    assert stub.calls == []


# ---- 4. Handle ------------------------------------------------------------------------------------------------------------

class Thing(_lib.Handle):
    _destroy = "mi_prep_destroy"

    def __init__(self, address=0x1000):
        self._h = C.c_void_p(address)


def test_handle_closes_once(stub):
    t = Thing()
    assert t._handle().value == 0x1000
    t.close()
    t.close()
    assert [(n, a[0].value) for n, a in stub.calls] == [("mi_prep_destroy", 0x1000)]
    with pytest.raises(ValueError, match="the Thing is closed"):
        t._handle()


def test_handle_is_a_context_manager(stub):
    with Thing() as t:
        assert stub.calls == []
    assert len(stub.calls) == 1
    with pytest.raises(ValueError, match="the .* is closed"):
        t._handle()


def test_handle_never_opened(stub):
    t = Thing(0)                                               # a constructor that failed: NULL
    with pytest.raises(ValueError, match="the .* is closed"):
        t._handle()
    t.close()
    u = Thing.__new__(Thing)                                   # what ExpressionMatrix._adopt starts from
    with pytest.raises(ValueError, match="the .* is closed"):
        u._handle()
    del u
    gc.collect()
    assert stub.calls == []


def test_handle_del_swallows_a_failing_destroy(monkeypatch):
    seen = []

    class Failing:
        def mi_prep_destroy(self, h):
            seen.append(h.value)
            raise RuntimeError("destroy failed")
    monkeypatch.setattr(_lib, "_lib", Failing())
    t = Thing()
    del t
    gc.collect()
    assert seen == [0x1000]
    with pytest.raises(RuntimeError):                          # close() itself does not hide it
        Thing().close()


# ---- 5. the package holds no conversion of its own ---------------------------------------------------------------------------

def test_only_lib_converts():
    for name in sorted(os.listdir(PKG)):
        if name.endswith(".py") and name != "_lib.py":
            src = open(os.path.join(PKG, name)).read()
            for idiom in ("data_as(", "byref(", ".mi_", "_lib.check("):
                assert idiom not in src, "%s holds %r" % (name, idiom)
