"""The cases of the batched energy kernels (K4, csrc/energy_kernels.hip: mi_energy_dense_f32 / _f32_ex / _f64), shared by
tests/test_energy_cases.py, which shows on the CPU that every case stays inside the limits of exact arithmetic and gets the
launch it is named for, and tests/test_gpu_energy_kernel.py, which holds the device to the reference BIT FOR BIT.
TEST INFRASTRUCTURE ONLY.

The criterion.  Let every entry of Q be an integer multiple of a grid g = 2^-k with |q| <= amax g, and the offset a multiple
of g or of a finer dyadic grid g' (FP64_GRID = 2^-6 for every case here).  In units of g:
  * a product q x with x in {0, 1} is q or 0: exact;
  * the MFMA form's fp32 accumulator of a 128 x 128 block is an fmaf chain of at most 128 such terms: every partial sum is an
    integer of at most 128 amax, exact in fp32 while that is below 2^24;
  * the 16-way fp32 tree over the masked accumulators of a lane holds integers of at most 16 * 128 amax: exact below 2^24;
  * the folds into fp64 (times 1 or 2), the wavefront shuffle, the fp64 atomics onto the offset and the VALU form's fp64
    sums hold multiples of g' of at most (sum |q| + |offset|) / g' of them: exact below 2^53, in ANY order.
So with 128 * 16 * amax < 2^24 and (sum |q| + |offset|) / g' < 2^53 every form must return the exact energy, whatever the
launch and the order of its atomics: one missing term, one wrong block weight or one stale mask word changes an integer
and is seen.

The launch (``plan``, a mirror of csrc/mi_energy_plan.h, checked against the host program's print-out in
tests/test_energy_plan_host.py): T = ceil(n / 128) block rows, S = T (T + 1) / 2 blocks (I, K >= I) row by row, rtiles =
ceil(R / 128) state tiles, the block list cut into ``pieces`` ranges [S p / pieces, S (p + 1) / pieces), one workgroup per
(piece, state tile): U = pieces * rtiles, renumbered across the 8 XCDs when U % 8 == 0."""
import collections
import functools

import numpy as np

TILE = 128
CUS_MI355X = 256
TREE = 16                          # masked accumulator values a lane adds in fp32 before the fold into fp64
FP64_GRID = 2.0 ** -6              # every entry of every fp32 case and every offset is a multiple of it
OFFSETS = (0.0, 0.5, -2.0)

Plan = collections.namedtuple("Plan", "T rtiles S pieces ranges U")


# ---- the launch -----------------------------------------------------------------------------------------------------

def pieces_of(T, rtiles, cus):
    resident = 2 * (cus if cus > 0 else 256)
    S = T * (T + 1) // 2
    pieces, best = 1, 0.0
    for rounds in range(1, 5):
        p = min(max(rounds * resident // rtiles, 1), S)
        units, longest = p * rtiles, -(-S // p)
        fill = float(S * rtiles) / float(-(-units // resident) * resident * longest)
        if fill > best + 0.02:
            best, pieces = fill, p
        if p == S:
            break
    return pieces


def plan(n, R, cus=CUS_MI355X):
    T, rtiles = -(-n // TILE), -(-R // TILE)
    S = T * (T + 1) // 2
    pieces = pieces_of(T, rtiles, cus)
    ranges = tuple((S * p // pieces, S * (p + 1) // pieces) for p in range(pieces))
    return Plan(T, rtiles, S, pieces, ranges, pieces * rtiles)


def triangle(T):
    """the blocks (I, K) in the kernel's order"""
    return [(I, K) for I in range(T) for K in range(I, T)]


def row_changes_inside(T, s0, s1):
    """how often a walk of blocks s0 .. s1 - 1 goes on to a block of the next row (where the kernel swaps its mask buffer)"""
    tri = triangle(T)
    return sum(1 for s in range(s0, s1 - 1) if tri[s + 1][0] != tri[s][0])


def _lengths(p):
    return [s1 - s0 for s0, s1 in p.ranges]


# property name -> the conditions a plan must meet, each with its wording; ``missing`` lists those it does not
PROPERTIES = {
    "single_block": lambda n, R, p: [
        ("one block", p.S == 1 and p.pieces == 1 and p.ranges == ((0, 1),)),
    ],
    "one_piece": lambda n, R, p: [
        ("whole triangle in one piece", p.pieces == 1 and p.S >= 3 and p.ranges == ((0, p.S),)),
        ("a row change inside the piece", row_changes_inside(p.T, 0, p.S) >= 1),
        ("ragged last tile", n % TILE != 0),
    ],
    "one_piece_two_row_changes": lambda n, R, p: [
        ("whole triangle in one piece", p.pieces == 1 and p.S >= 6 and p.ranges == ((0, p.S),)),
        ("two row changes inside the piece", row_changes_inside(p.T, 0, p.S) >= 2),
        ("ragged last tile", n % TILE != 0),
    ],
    "block_pieces_no_remap": lambda n, R, p: [
        ("one block per piece", p.pieces == p.S > 1 and set(_lengths(p)) == {1}),
        ("no XCD remap with several units", p.U % 8 != 0 and p.U > 1),
    ],
    "block_pieces_remap": lambda n, R, p: [
        ("one block per piece", p.pieces == p.S > 1 and set(_lengths(p)) == {1}),
        ("XCD remap", p.U % 8 == 0 and p.U > 8),
    ],
    "multi_block_remap": lambda n, R, p: [
        ("XCD remap", p.U % 8 == 0 and p.U > 8),
        ("several pieces of two blocks or more", p.pieces > 1 and min(_lengths(p)) >= 2),
        ("a piece that starts mid-row", any(triangle(p.T)[s0][0] != triangle(p.T)[s0][1] for s0, _ in p.ranges)),
        ("a piece of three blocks or more that crosses a row",
         any(s1 - s0 >= 3 and row_changes_inside(p.T, s0, s1) >= 1 for s0, s1 in p.ranges)),
    ],
}


def missing(prop, n, R, cus):
    """the conditions of ``prop`` that the launch of (n, R) on ``cus`` compute units does not meet, by name"""
    return ["%s (n = %d, R = %d, %d CUs): %s" % (prop, n, R, cus, what)
            for what, ok in PROPERTIES[prop](n, R, plan(n, R, cus)) if not ok]


# (property, n, R); R of the single-block cases at the edges of the 64-state tiles of the transpose
CASES = (
    ("single_block", 1, 1),
    ("single_block", 127, 63),
    ("single_block", 128, 64),
    ("single_block", 128, 65),
    ("single_block", 64, 129),
    ("one_piece", 129, 3),
    ("one_piece_two_row_changes", 300, 70),
    ("block_pieces_no_remap", 385, 130),
    ("block_pieces_remap", 513, 1024),
    ("multi_block_remap", 641, 8192),
)
ISOLATION = (300, 70)              # block isolation: T = 3, every block (I, K) on its own
BIG_N = (1, 63, 64, 65, 300)       # the fp64 form: wavefront edges of the column loop
BIG_R = (1, 3, 4, 5)               # ... and the four-waves-per-workgroup edge


def case_id(case):
    return "%s-n%d-R%d" % case


# ---- the matrices and the states -----------------------------------------------------------------------------------

def _ro(a):
    a.setflags(write=False)
    return a


def _sym_int(rng, n, amax):
    A = rng.integers(-amax, amax + 1, size=(n, n), dtype=np.int64)
    return np.triu(A) + np.triu(A, 1).T


INT_AMAX, DYADIC_AMAX, DYADIC_GRID = 64, 16 * 64, 2.0 ** -6


@functools.lru_cache(maxsize=None)
def integer_sym(n, seed, amax=INT_AMAX):
    """symmetric, integer entries in [-amax, amax], float32"""
    return _ro(np.ascontiguousarray(_sym_int(np.random.default_rng([1, n, seed]), n, amax).astype(np.float32)))


@functools.lru_cache(maxsize=None)
def dyadic_sym(n, seed):
    """symmetric, entries multiples of 2^-6 with |q| <= 16, float32"""
    A = _sym_int(np.random.default_rng([2, n, seed]), n, DYADIC_AMAX)
    return _ro(np.ascontiguousarray((A * DYADIC_GRID).astype(np.float32)))


@functools.lru_cache(maxsize=None)
def block_only(n, I, K, seed):
    """integer entries (|q| <= 64, none zero) in the 128 x 128 block (I, K) and its mirror image, zero elsewhere"""
    assert I <= K
    rng = np.random.default_rng([3, n, I, K, seed])
    A = _sym_int(rng, n, INT_AMAX)
    A[A == 0] = 1
    blk = np.zeros((n, n), dtype=bool)
    blk[I * TILE:(I + 1) * TILE, K * TILE:(K + 1) * TILE] = True
    return _ro(np.ascontiguousarray(np.where(blk | blk.T, A, 0).astype(np.float32)))


BIG_AMAX = 2 ** 30


@functools.lru_cache(maxsize=None)
def big_int_f64(n, seed):
    """symmetric float64 integers up to 2^30 in size; every diagonal entry is odd and above 2^24 (so is about half of the
    rest): not representable in float32"""
    rng = np.random.default_rng([4, n, seed])
    A = _sym_int(rng, n, BIG_AMAX)
    d = (2 ** 24 + 1 + 2 * rng.integers(0, 2 ** 28, size=n)) * rng.choice([-1, 1], size=n)
    A[np.arange(n), np.arange(n)] = d
    return _ro(np.ascontiguousarray(A.astype(np.float64)))


@functools.lru_cache(maxsize=None)
def states(n, R, seed):
    """[R, n] bytes: density-0.5 random rows, and as far as R allows (in this order, from the last row backwards) a row of
    all ones, a row of all zeros and a row with a single one in the last cell; at least one random row from R = 2 on"""
    X = (np.random.default_rng([5, n, R, seed]).random((R, n)) < 0.5).astype(np.uint8)
    X[R - 1] = 1
    if R >= 3:
        X[R - 2] = 0
    if R >= 4:
        X[R - 3] = 0
        X[R - 3, n - 1] = 1
    return _ro(X)


# ---- the reference and its limits ----------------------------------------------------------------------------------

def reference(Q, X, offset=0.0):
    """E_r = x_r^T Q x_r + offset in float64"""
    Xd = np.asarray(X, dtype=np.float64)
    return ((Xd @ np.asarray(Q, dtype=np.float64)) * Xd).sum(axis=1) + float(offset)


def reference_int(Q, X, offset, grid=FP64_GRID):
    """the same in int64, in units of ``grid``"""
    Qi = np.asarray(Q, dtype=np.float64) / grid
    assert np.array_equal(Qi, np.rint(Qi)) and float(offset / grid).is_integer()
    Qi, Xi = Qi.astype(np.int64), np.asarray(X, dtype=np.int64)
    return ((Xi @ Qi) * Xi).sum(axis=1) + int(offset / grid)


def exactness(Q, offset, grid, fp64_grid=FP64_GRID):
    """(amax in units of ``grid``, bound on |E| in units of ``fp64_grid``) of a matrix whose entries are multiples of
    ``grid``: the two numbers the criterion limits (TILE * TREE * amax < 2^24 for the fp32 forms, the bound < 2^53 for all)"""
    Qu = np.abs(np.asarray(Q, dtype=np.float64)) / grid
    assert np.array_equal(Qu, np.rint(Qu)), "an entry is off the grid"
    assert float(grid / fp64_grid).is_integer() and float(offset / fp64_grid).is_integer()
    return int(Qu.max()), int(Qu.sum() * (grid / fp64_grid)) + int(abs(offset) / fp64_grid)
