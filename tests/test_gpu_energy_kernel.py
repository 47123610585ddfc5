"""The batched energy kernels (K4, csrc/energy_kernels.hip) held to EXACT energies.  With matrix entries on a dyadic grid
and of bounded size every fp32 product, fmaf chain and tree, every fp64 fold and every fp64 atomic of the kernels is exact
(tests/energy_cases.py states the conditions, tests/test_energy_cases.py shows every case meets them), so the VALU form,
the MFMA form and the fp64 form must each equal the float64 reference bit for bit, whatever the launch and the order of
the atomics.  Every case first certifies, from the CPU mirror of the launch at THIS device's CU count, that it still gets
the launch it is named for (one block; the whole triangle in one piece; one block per piece with and without the XCD remap;
multi-block pieces under the remap): a planner change that empties a case fails it by name."""
import ctypes as C

import numpy as np
import pytest

import energy_cases as ec
from scrna_seq_qannealing_clustering_amd import _lib, engine
from test_gpu_parity import random_sym

pytestmark = pytest.mark.gpu

SEED = 0
MI_EINVAL = -1
BUILDERS = {"integer": ec.integer_sym, "dyadic": ec.dyadic_sym}


def cus():
    return _lib.device_info(0)["compute_units"]


def differing(got, want):
    bad = np.flatnonzero(got != want)
    return "%d of %d states differ, first %s: got %s, want %s" % (
        len(bad), len(want), bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())


def assert_exact(got, want, what):
    assert got.dtype == np.float64 and np.array_equal(got, want), "%s: %s" % (what, differing(got, want))


@pytest.mark.parametrize("kind", sorted(BUILDERS))
@pytest.mark.parametrize("case", ec.CASES, ids=ec.case_id)
def test_every_form_is_exact(case, kind):
    prop, n, R = case
    wrong = ec.missing(prop, n, R, cus())
    assert not wrong, wrong
    Q, X = BUILDERS[kind](n, SEED), ec.states(n, R, SEED)
    Qd = Q.astype(np.float64)
    base = ec.reference(Q, X)                                        # exact, and so is base + offset (test_energy_cases.py)
    for offset in ec.OFFSETS:
        want = base + offset
        what = "%s, %s Q, offset %g" % (ec.case_id(case), kind, offset)
        assert_exact(engine.energy_dense(Q, X, offset=offset, path=1), want, what + ", VALU (path 1)")
        mfma = engine.energy_dense(Q, X, offset=offset, path=2)
        assert_exact(mfma, want, what + ", MFMA (path 2)")
        assert_exact(engine.energy_dense_f64(Qd, X, offset=offset), want, what + ", fp64 form")
        assert engine.energy_dense(Q, X, offset=offset, path=2).tobytes() == mfma.tobytes(), what + ": two MFMA calls differ"


def test_each_block_alone_is_exact_on_the_mfma_form():
    """one 128 x 128 block (and its mirror image) of Q filled at a time: a wrong weight, a block taken for another or a mirror
    image left out is named"""
    n, R = ec.ISOLATION
    T = ec.plan(n, R, cus()).T
    assert T == 3
    X = ec.states(n, R, SEED)
    wrong = []
    for I, K in ec.triangle(T):
        Q = ec.block_only(n, I, K, SEED)
        want = ec.reference(Q, X, 0.5)
        for path in (2, 1):
            got = engine.energy_dense(Q, X, offset=0.5, path=path)
            if not np.array_equal(got, want):
                wrong.append("block (I = %d, K = %d), path %d: %s" % (I, K, path, differing(got, want)))
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("offset", [0.0, 0.5])
def test_identity_states_return_the_diagonal_bit_for_bit(offset):
    """X = I on full-mantissa floats: state r holds the single term Q[r][r], so every form returns float64(Q[r][r]) + offset
    with its one rounding; a row / column or tile mapping slip that a symmetric-looking sum hides moves another entry in"""
    n = 300
    Q = random_sym(n, 77)
    X = np.eye(n, dtype=np.uint8)
    want = Q.diagonal().astype(np.float64) + offset
    assert len(np.unique(want)) == n
    for path in (1, 2):
        assert_exact(engine.energy_dense(Q, X, offset=offset, path=path), want, "path %d" % path)
    assert_exact(engine.energy_dense(Q, X, offset=offset), want, "auto path")
    assert_exact(engine.energy_dense_f64(Q.astype(np.float64), X, offset=offset), want, "fp64 form")


@pytest.mark.parametrize("n", ec.BIG_N)
def test_fp64_form_does_not_narrow_to_fp32(n):
    Q = ec.big_int_f64(n, SEED)
    assert (Q.astype(np.float32).astype(np.float64) != Q).any()
    for R in ec.BIG_R:
        X = ec.states(n, R, SEED)
        for offset in (0.0, 0.5):
            assert_exact(engine.energy_dense_f64(Q, X, offset=offset), ec.reference(Q, X, offset), "n = %d, R = %d" % (n, R))


def test_auto_path_is_the_valu_form_below_32_states_and_the_mfma_form_from_32():
    """full-mantissa Q at n = 100 (one block, one unit: the MFMA form has a single summation order).  R = 31: the VALU
    form's bytes.  R = 32: the MFMA form's, which on such a matrix are not the VALU form's."""
    Q = random_sym(100, 5)
    X = ec.states(100, 32, SEED)
    assert engine.energy_dense(Q, X[:31], offset=0.5).tobytes() == engine.energy_dense(Q, X[:31], offset=0.5, path=1).tobytes()
    auto, mfma = engine.energy_dense(Q, X, offset=0.5), engine.energy_dense(Q, X, offset=0.5, path=2)
    assert np.array_equal(auto, mfma) or np.allclose(auto, mfma, rtol=1e-12)        # (the bar of test_energy_kernel_parity)
    assert auto.tobytes() == mfma.tobytes() and auto.tobytes() != engine.energy_dense(Q, X, offset=0.5, path=1).tobytes()


# ---- state bytes other than 0 / 1 -----------------------------------------------------------------------------------

def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _call_f32(Q, X, path):
    out = np.full(len(X), np.nan)
    rc = _lib.load().mi_energy_dense_f32_ex(_ptr(Q, C.c_float), len(Q), _ptr(X, C.c_uint8), len(X), 0.5, _ptr(out, C.c_double), 0,
                                            path, None)
    return rc, _lib.load().mi_last_error().decode(), out


def _call_f64(Q, X):
    out = np.full(len(X), np.nan)
    rc = _lib.load().mi_energy_dense_f64(_ptr(Q, C.c_double), len(Q), _ptr(X, C.c_uint8), len(X), 0.5, _ptr(out, C.c_double), 0)
    return rc, _lib.load().mi_last_error().decode(), out


@pytest.mark.parametrize("byte", [2, 255])
def test_a_state_byte_other_than_0_or_1_is_refused_on_every_path(byte):
    """the VALU form takes any non-zero byte as set, the MFMA form multiplies by the byte's value and masks with its bit 0:
    such a batch had energies that depended on the path.  Refused with the cell and the state named; the next valid call
    on the same entry works."""
    n, R = 130, 40
    Q, good = ec.integer_sym(n, SEED), ec.states(n, R, SEED)
    Qd = np.ascontiguousarray(Q.astype(np.float64))
    bad = good.copy()
    bad[R - 2, 129] = byte                                           # in the all-zeros state: the last cell, the second block row
    want = ec.reference(Q, good, 0.5)
    for path in (0, 1, 2):
        rc, msg, out = _call_f32(Q, bad, path)
        assert rc == MI_EINVAL and "cell 129 of state %d is %d" % (R - 2, byte) in msg, (path, rc, msg)
        assert np.isnan(out).all()
        rc, msg, out = _call_f32(Q, good, path)
        assert rc == _lib.MI_OK and np.array_equal(out, want), (path, rc, msg)
    rc, msg, out = _call_f64(Qd, bad)
    assert rc == MI_EINVAL and "cell 129 of state %d is %d" % (R - 2, byte) in msg and np.isnan(out).all(), (rc, msg)
    rc, msg, out = _call_f64(Qd, good)
    assert rc == _lib.MI_OK and np.array_equal(out, want), (rc, msg)


def test_spins_cast_to_bytes_are_refused_by_the_python_entry():
    """+-1 spins through engine.energy_dense's uint8 cast arrive as 1 and 255"""
    Q = ec.integer_sym(130, SEED)
    spins = 2 * ec.states(130, 40, SEED).astype(np.int8) - 1
    for path in (0, 1, 2):
        with pytest.raises(_lib.MiSaError, match="states must be bytes 0 or 1"):
            engine.energy_dense(Q, spins, path=path)
    with pytest.raises(_lib.MiSaError, match="states must be bytes 0 or 1"):
        engine.energy_dense_f64(Q.astype(np.float64), spins)
