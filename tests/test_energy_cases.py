"""tests/energy_cases.py without a GPU: every case of tests/test_gpu_energy_kernel.py stays inside the limits within which
the kernels' arithmetic is exact (so "bit for bit" is the right bar, and the float64 reference is itself exact: it equals an
int64 evaluation), every matrix is what its builder says, and every case gets the launch it is named for on 256 compute
units, so that a GPU run cannot pass vacuously."""
import numpy as np
import pytest

import energy_cases as ec

SEED = 0
F32_BUILDERS = {"integer": (ec.integer_sym, 1.0, ec.INT_AMAX), "dyadic": (ec.dyadic_sym, ec.DYADIC_GRID, ec.DYADIC_AMAX)}


# ---- 1. the launches ------------------------------------------------------------------------------------------------

def test_every_case_gets_the_launch_it_is_named_for_on_256_cus():
    wrong = [m for prop, n, R in ec.CASES for m in ec.missing(prop, n, R, 256)]
    assert not wrong, wrong


def test_the_plans_of_the_case_list_on_256_cus():
    """the figures the cases were chosen by"""
    got = {(n, R): ec.plan(n, R, 256) for _, n, R in ec.CASES}
    for n, R in ((1, 1), (127, 63), (128, 64), (128, 65), (64, 129)):
        assert got[n, R].S == 1 and got[n, R].pieces == 1
    assert [R for p, _, R in ec.CASES if p == "single_block"] == [1, 63, 64, 65, 129]       # around the 64-state transpose tiles
    assert (got[64, 129].rtiles, got[64, 129].U) == (2, 2)
    assert (got[129, 3].S, got[129, 3].pieces) == (3, 1) and (got[300, 70].S, got[300, 70].pieces) == (6, 1)
    assert (got[385, 130].pieces, got[385, 130].U) == (10, 20)
    assert (got[513, 1024].pieces, got[513, 1024].U) == (15, 120)
    p = got[641, 8192]
    assert (p.S, p.pieces, p.U) == (21, 8, 512) and sorted(set(s1 - s0 for s0, s1 in p.ranges)) == [2, 3]
    assert ec.plan(*ec.ISOLATION, 256).T == 3
    assert max(n * R for _, n, R in ec.CASES) == 641 * 8192                               # 5.3 MB of states at the most


def test_a_property_that_is_missing_is_named():
    """what the GPU test prints when a device's CU count empties a case: (300, 70) is one piece only while 6 units do not
    fill 2 % of the chip; the remap cases without the remap"""
    assert ec.missing("one_piece_two_row_changes", 300, 70, 256) == []
    m = ec.missing("one_piece_two_row_changes", 300, 70, 64)
    assert len(m) == 1 and "whole triangle in one piece" in m[0] and "64 CUs" in m[0]
    assert any("XCD remap" in w for w in ec.missing("block_pieces_remap", 385, 130, 256))
    assert any("starts mid-row" in w or "two blocks" in w for w in ec.missing("multi_block_remap", 513, 1024, 256))


def test_row_changes_and_triangle():
    assert ec.triangle(3) == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    assert ec.row_changes_inside(3, 0, 6) == 2 and ec.row_changes_inside(2, 0, 3) == 1
    assert ec.row_changes_inside(3, 0, 3) == 0 and ec.row_changes_inside(3, 2, 4) == 1


# ---- 2. the matrices and the states ---------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", sorted(F32_BUILDERS))
@pytest.mark.parametrize("case", ec.CASES, ids=ec.case_id)
def test_fp32_cases_are_inside_the_exactness_limits(case, kind):
    _, n, R = case
    build, grid, amax_want = F32_BUILDERS[kind]
    Q = build(n, SEED)
    X = ec.states(n, R, SEED)
    assert Q.dtype == np.float32 and Q.shape == (n, n) and np.array_equal(Q, Q.T) and not Q.flags.writeable
    assert X.dtype == np.uint8 and X.shape == (R, n) and X.max() <= 1
    assert X[R - 1].all() and (R < 3 or not X[R - 2].any()) and (R < 4 or (X[R - 3].sum() == 1 and X[R - 3, n - 1] == 1))
    if R >= 2 and n >= 64:
        assert 0.3 < X[0].mean() < 0.7
    if n >= 64:
        assert np.abs(Q).max() == amax_want * grid                    # the builder reaches its bound
    for offset in ec.OFFSETS:
        amax, bound = ec.exactness(Q, offset, grid)
        assert amax <= amax_want and ec.TILE * ec.TREE * amax < 2 ** 24           # fp32 chain and tree
        assert bound < 2 ** 53                                                    # fp64 folds and atomics
        if n <= 300:
            want = ec.reference_int(Q, X, offset)
            got = ec.reference(Q, X, offset)
            assert np.array_equal(got / ec.FP64_GRID, want.astype(np.float64)) and np.abs(want).max() <= bound


def test_the_largest_reference_equals_int64_on_a_slice_of_its_states():
    """(641, 8192) is above the n <= 300 of the int64 check: 256 of its states, the special rows among them"""
    Q, X = ec.dyadic_sym(641, SEED), ec.states(641, 8192, SEED)[-256:]
    assert np.array_equal(ec.reference(Q, X, 0.5) / ec.FP64_GRID, ec.reference_int(Q, X, 0.5).astype(np.float64))


def test_block_only_matrices_fill_one_block_and_its_mirror():
    n, R = ec.ISOLATION
    T = ec.plan(n, R).T
    X = ec.states(n, R, SEED)
    for I, K in ec.triangle(T):
        Q = ec.block_only(n, I, K, SEED)
        assert Q.dtype == np.float32 and np.array_equal(Q, Q.T)
        nz = Q != 0
        rows, cols = slice(I * 128, (I + 1) * 128), slice(K * 128, (K + 1) * 128)
        assert nz[rows, cols].all()
        nz[rows, cols] = False
        nz[cols, rows] = False
        assert not nz.any()
        amax, bound = ec.exactness(Q, 0.5, 1.0)
        assert ec.TILE * ec.TREE * amax < 2 ** 24 and bound < 2 ** 53
        assert np.array_equal(ec.reference(Q, X, 0.5) / ec.FP64_GRID, ec.reference_int(Q, X, 0.5).astype(np.float64))
    # the energies of two blocks differ on some state: a block taken for another is seen
    assert not np.array_equal(ec.reference(ec.block_only(n, 0, 1, SEED), X), ec.reference(ec.block_only(n, 0, 2, SEED), X))


@pytest.mark.parametrize("n", ec.BIG_N)
def test_big_fp64_matrices_are_exact_in_fp64_and_not_in_fp32(n):
    Q = ec.big_int_f64(n, SEED)
    assert Q.dtype == np.float64 and np.array_equal(Q, Q.T) and np.array_equal(Q, np.rint(Q))
    lossy = Q.astype(np.float32).astype(np.float64) != Q
    assert lossy.diagonal().all() and lossy.sum() >= (n * n) // 4
    assert (np.abs(Q.diagonal()) > 2 ** 24).all() and (Q.diagonal() % 2 == 1).all()
    amax, bound = ec.exactness(Q, 0.5, 1.0)
    assert amax <= ec.BIG_AMAX and bound < 2 ** 53
    for R in ec.BIG_R:
        X = ec.states(n, R, SEED)
        want = ec.reference_int(Q, X, 0.5)
        assert np.array_equal(ec.reference(Q, X, 0.5) / ec.FP64_GRID, want.astype(np.float64))
        # the float32 rounding of Q would be seen: it moves the energy of the all-ones state
        assert ec.reference(Q.astype(np.float32), X, 0.5)[R - 1] != ec.reference(Q, X, 0.5)[R - 1]
