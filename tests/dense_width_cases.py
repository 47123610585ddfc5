"""The cases that run the dense QUBO chain at EVERY register width and at the edges of the large-model kernels, shared by
tests/test_dense_width_cases.py -- which shows without a GPU that every width and ring depth occurs and that no case is
vacuous on the oracle alone -- and tests/test_gpu_dense_widths.py / tests/test_gpu_dense_xl_edges.py, which hold the device
to the oracle on them.  TEST INFRASTRUCTURE ONLY.

Up to 4096 variables the chain keeps a replica's fields in the registers of one wavefront, NT = 4, 8, .. 64 fields a lane
(csrc/dense_kernels.hip; width()), as K1 (k_anneal_dense<NT>), K1w (k_anneal_dense_wg<NT,GR>: 16 replicas share the rows of
Q through an LDS ring of U units of GR rows, ring_depth()) and, up to NT = 44, K1m (k_anneal_dense_mfma<NT>).  This module
restates those formulas and derives from them, per (size, variant, unit_rows), the kernel a run must report or that it is
refused (expected()).

Above 4096 variables K1x (k_anneal_dense_xl<CH>, CH chunks of 4096 columns) and K1g (k_xg_diag / k_xg_chain / k_xg_panel:
blocks of 64 rows in groups of eight, 64 replicas a range, 256 columns a pass workgroup) take over; xl_model() and the
B* tables below are their cases."""
import dataclasses
import functools

import numpy as np

from oracle import sa_oracle as so
from test_gpu_parity import E_RTOL, random_sym          # noqa: F401  (the project's energy bar and dense test matrix)

# ---- A: every width below 4097 variables -------------------------------------------------------------------------------
R, SEED, REPLICA_OFFSET, RESYNC = 19, 7, 5, 3            # 19 replicas: a ragged K1 block (4 a block) and K1w workgroup (16)
BETAS = np.geomspace(0.05, 4.0, 5)
BETAS.setflags(write=False)
SCENARIOS = ("random", "init")                           # the chain's own random start / a given one with re-synchronisation
FULL = tuple(256 * k - 37 for k in range(1, 17))         # 4 k slots, the last one of 27 variables: NT = 4 k
EXTRA = (1281, 2816, 2817, 3841, 4096)                   # three wholly padded slots at NT = 24 / 48 / 64; the last K1m size; every lane live
SIZES = tuple(sorted(FULL + EXTRA))
WIDTHS = tuple(range(4, 65, 4))
MAX_MFMA_NT = 44                                         # kMaxMfmaNT
LDS_RING_BYTES = 160 * 1024 - 256                        # kLdsBytes
VARIANTS = ((1, 0), (2, 2), (2, 4), (3, 0))              # (variant, unit_rows) of a run


def slots(n):
    return (n + 63) // 64


def width(n):
    """NT: fields per lane, the slots rounded up to a multiple of four."""
    return 4 * ((slots(n) + 3) // 4)


def ring_depth(nt, gr):
    """WgCfg<NT,GR>::U: what fits into LDS, capped so that (U - 2) * GR stays within the 6-bit vmcnt."""
    return min(LDS_RING_BYTES // (gr * nt * 256), 2 + 60 // gr)


def ring_ok(nt, gr):
    return ring_depth(nt, gr) >= 3 and 64 % gr == 0


def ring_class(nt, gr):
    """'refused' (fewer than 3 units fit), 'cap' (the vmcnt cap binds), 'min' (U = 3) or 'fit'."""
    if not ring_ok(nt, gr):
        return "refused"
    if ring_depth(nt, gr) == 2 + 60 // gr:
        return "cap"
    return "min" if ring_depth(nt, gr) == 3 else "fit"


def auto_unit_rows(nt):
    """The ring unit the library takes when none is asked for: 4 rows, 2 where 4 do not fit."""
    return 4 if ring_ok(nt, 4) else 2


def expected(n, variant, unit_rows=0):
    """The kernel name a one-launch run of the variant reports; None: the run is refused (MI_EUNSUPPORTED, -5)."""
    nt = width(n)
    if variant == 1:
        return "k_anneal_dense<%d>" % nt
    if variant == 2:
        gr = unit_rows or auto_unit_rows(nt)
        return "k_anneal_dense_wg<%d,%d>" % (nt, gr) if ring_ok(nt, gr) else None
    if variant == 3:
        return "k_anneal_dense_mfma<%d>" % nt if nt <= MAX_MFMA_NT else None
    raise ValueError(variant)


EUNSUPPORTED = -5


@functools.lru_cache(maxsize=4)
def matrix(n):
    Qs = random_sym(n, 1000 + n)
    Qs.setflags(write=False)
    return Qs


@functools.lru_cache(maxsize=None)
def given_start(n, reps=R):
    init = np.random.RandomState(n).randint(0, 2, size=(reps, n)).astype(np.uint8)
    init.setflags(write=False)
    return init


def run_kwargs(n, scenario, reps=R):
    """What a scenario adds to Problem.anneal (the oracle takes ``init`` for ``initial_states``)."""
    if scenario == "init":
        return dict(replica_offset=REPLICA_OFFSET, initial_states=given_start(n, reps), resync_interval=RESYNC)
    return dict(replica_offset=REPLICA_OFFSET)


def oracle(n, scenario, betas=BETAS, reps=R, **over):
    kw = run_kwargs(n, scenario, reps)
    kw["init"] = kw.pop("initial_states", None)
    kw.update(over)
    st, en, stats = so.sa_dense_philox(matrix(n), reps, betas, SEED, **kw)
    return st, en, int(stats[0]), int(stats[1])


@dataclasses.dataclass(frozen=True)
class Reference:
    states: np.ndarray
    energies: np.ndarray
    proposals: int
    accepted: int


def _frozen(st, en, prop, acc):
    st.setflags(write=False)
    en.setflags(write=False)
    return Reference(st, en, prop, acc)


@functools.lru_cache(maxsize=None)
def reference(n, scenario):
    """The oracle's run of a (model, scenario), once per session and left unchanged."""
    return _frozen(*oracle(n, scenario))


# the library's own choice above the K1m sizes: 40 replicas (K1w from 32 up), 8 sweeps in launches of 3, 3 and 2
AUTO_SIZES = (2817, 4096)                                # NT = 48 (GR = 4, U = 3) and NT = 64 (GR = 2: 4 rows do not fit)
AUTO_R, AUTO_CHUNK, AUTO_RESYNC = 40, 3, 5
AUTO_BETAS = np.geomspace(0.05, 4.0, 8)
AUTO_BETAS.setflags(write=False)


@functools.lru_cache(maxsize=None)
def auto_reference(n):
    st, en, stats = so.sa_dense_philox(matrix(n), AUTO_R, AUTO_BETAS, SEED, replica_offset=REPLICA_OFFSET, resync_interval=AUTO_RESYNC)
    return _frozen(st, en, int(stats[0]), int(stats[1]))


# ---- B: the large-model edges ------------------------------------------------------------------------------------------
XL_RTOL, XL_ATOL = 1e-5, 1e-3                            # energies from cached fp32 fields against the oracle's fp64 sum
XG_RTOL = 1e-6                                           # K1g's energies against K1x's
K1X, K1G_FUSED, K1G_BLOCK = (2, 0), (1, 2), (1, 1)       # (xl_batched, xl_chain)
XL_FORMS = ((K1X, "k_anneal_dense_xl"), (K1G_FUSED, "k_xg_chain + k_xg_panel"), (K1G_BLOCK, "k_xg_diag + k_xg_panel"))
XG_BLOCK, XG_GROUP, XG_COLS, XG_REPS, XL_CHUNK = 64, 8, 256, 64, 4096
XL_SEED, XL_OFFSET = 11, 5


@functools.lru_cache(maxsize=2)
def xl_model(n, seed=None):
    """2 % of the pairs coupled with uniform(-0.5, 0.5), symmetric; the diagonal uniform in [2, 3]: at a cold temperature an
    all-zero state accepts nothing and a lone one flips back (the fields of the zeros stay above 1)."""
    rng = np.random.RandomState(n if seed is None else seed)
    Qs = np.zeros((n, n), dtype=np.float32)
    count = n * n // 50                                  # drawn as (i, j) of the square: 2 % of the pairs i < j are kept
    iu, ju = rng.randint(0, n, size=count), rng.randint(0, n, size=count)
    Qs[iu, ju] = rng.rand(count).astype(np.float32) - np.float32(0.5)
    Qs = np.triu(Qs, 1)
    Qs = np.ascontiguousarray(Qs + Qs.T)
    Qs[np.arange(n), np.arange(n)] = (2.0 + rng.rand(n)).astype(np.float32)
    Qs.setflags(write=False)
    return Qs


def xl_shape(n):
    """(blocks, groups, blocks of the last group, variables of the last block, 256-column ranges, ncols == n, K1x chunks)."""
    nb = (n + XG_BLOCK - 1) // XG_BLOCK
    ng = (nb + XG_GROUP - 1) // XG_GROUP
    ncols = (n + XG_COLS - 1) // XG_COLS * XG_COLS
    return nb, ng, nb - XG_GROUP * (ng - 1), n - XG_BLOCK * (nb - 1), ncols // XG_COLS, ncols == n, (n + XL_CHUNK - 1) // XL_CHUNK


def xl_oracle(n, reps, betas, init=None, **kw):
    st, en, stats = so.sa_dense_philox(xl_model(n), reps, betas, XL_SEED, init=init, **kw)
    return _frozen(st, en, int(stats[0]), int(stats[1]))


# B1: group shapes.  65 full blocks (a last group of one); 68 = a last group of 4, ncols exact; 69 with one variable in the
# last; 72 = 9 full groups, ncols exact
B1_SIZES = (4160, 4352, 4353, 4608)
B1_R = 3
B1_BETAS = np.geomspace(0.3, 3.0, 3)
B1_RESYNC = 2


def xl_start(n, reps):
    init = np.random.RandomState(n + 1).randint(0, 2, size=(reps, n)).astype(np.uint8)
    init.setflags(write=False)
    return init


@functools.lru_cache(maxsize=None)
def b1_reference(n, scenario):
    if scenario == "init":
        return xl_oracle(n, B1_R, B1_BETAS, init=xl_start(n, B1_R), replica_offset=XL_OFFSET, resync_interval=B1_RESYNC)
    return xl_oracle(n, B1_R, B1_BETAS, replica_offset=XL_OFFSET)


# B2: the K1x chunk edge
B2_SIZES = (8192, 8193)
B2_R = 2
B2_BETAS = np.geomspace(0.3, 3.0, 2)


@functools.lru_cache(maxsize=None)
def b2_reference(n):
    return xl_oracle(n, B2_R, B2_BETAS, replica_offset=XL_OFFSET)


# B3: replica ranges.  One / two / five ranges of 64; 512 replicas = the last count on the fused chain by default
B3_N = 4160
B3_COUNTS = (64, 65, 257, 512, 513)
B3_BETAS = np.geomspace(0.3, 3.0, 2)


def b3_windows(reps):
    """(first replica, count) of the windows compared with the oracle: the first two, 62 .. 65 where they exist, the last two."""
    out = [(0, 2)]
    if reps > 62:
        out.append((62, min(4, reps - 62)))
    out.append((reps - 2, 2))
    return out


@functools.lru_cache(maxsize=None)
def b3_reference(lo, count):
    return xl_oracle(B3_N, count, B3_BETAS, replica_offset=lo)


# B4: dead and partly live replica ranges
B4_N, B4_R, B4_SWEEPS, B4_COLD = 4353, 192, 3, 1e4
B4_LIVE = {1: (1, 6), 2: (0,), 3: (7,), 8: (4,)}         # group -> its blocks that flip something in replicas 128 .. 191


def b4_planted():
    """[(replica, variable)] of the ones planted into replicas 128 .. 191.  Some replicas get none; no replica gets two in
    one block."""
    out = []
    for k in range(64):
        r = 128 + k
        if k % 2 == 0:
            out.append((r, 64 * 9 + k))                  # group 1, block 1
        if k % 3 == 0:
            out.append((r, 64 * 14 + 63 - k))            # group 1, block 6
        if k % 4 == 1:
            out.append((r, 64 * 16 + (7 * k) % 64))      # group 2, block 0
        if k % 5 == 2:
            out.append((r, 64 * 31 + k))                 # group 3, its last block
        if k in (0, 17, 63):
            out.append((r, B4_N - 1))                    # the last group's last block: its only variable
    return out


@functools.lru_cache(maxsize=None)
def b4_inputs():
    """(betas [192], init [192, n]): replicas 0 .. 63 hot to cold from a random start, 64 .. 127 cold from all zeros,
    128 .. 191 cold from all zeros but the planted ones."""
    betas = np.concatenate([np.geomspace(0.05, 5.0, 64), np.full(128, B4_COLD)])
    init = np.zeros((B4_R, B4_N), dtype=np.uint8)
    init[:64] = np.random.RandomState(B4_N).randint(0, 2, size=(64, B4_N))
    for r, i in b4_planted():
        init[r, i] = 1
    betas.setflags(write=False)
    init.setflags(write=False)
    return betas, init


@functools.lru_cache(maxsize=None)
def b4_reference():
    betas, init = b4_inputs()
    return xl_oracle(B4_N, B4_R, betas, init=init, num_sweeps=B4_SWEEPS)


# B5: a continued run with one temperature per replica
B5_N, B5_R = 4160, 65
B5_BETAS = np.geomspace(0.3, 3.0, 2)
B5_RUNG = np.geomspace(0.05, 5.0, B5_R)


@functools.lru_cache(maxsize=None)
def b5_reference():
    """(the first two sweeps, the run continued from their states at sweep 2 for two more with one beta per replica)."""
    first = xl_oracle(B5_N, B5_R, B5_BETAS, replica_offset=XL_OFFSET)
    return first, xl_oracle(B5_N, B5_R, B5_RUNG, init=first.states, replica_offset=XL_OFFSET, sweep_offset=2, num_sweeps=2)
