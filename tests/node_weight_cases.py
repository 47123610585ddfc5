"""The cases of the node-weighted Potts chain (chain 2d, mi_sa_problem_set_node_weights) shared by
tests/test_node_weight_cases.py, which shows on the CPU that every case is sharp -- moves accepted and rejected from the
first sweep to the last, and a chain that read the cluster sums frozen at the start of each 64-seat slot ending elsewhere --
and tests/test_gpu_node_weight_edges.py, which holds the device to the restatement on them.  TEST INFRASTRUCTURE ONLY.

A case is a kernel form x a label count x a weight pattern.  The forms: K3f (csrc/potts_fast_kernels.hip) with 8 and 16
label fields, with and without its threshold wavefront; K3 (csrc/sparse_kernels.hip) at D = 16, 32, 64 and in its
runtime-width form for rows wider than 64.  The patterns (PATTERNS): the quantised degrees of the modularity model, a third
of the weights zero, one node with half of a total of exactly 2^30, weights in {0, 1, 2}, and coefficients cw drawn
independently of the weights wq.  The reference is tests/test_modularity_model.py:chain2d on the model as the device
sweeps it; the seats of that layout are computed here without a GPU (potts_merge_cases.Layout) and the GPU test checks that
the problem it creates took the same ones."""
import dataclasses
import functools
import time
from typing import Optional, Tuple

import numpy as np

from conftest import load_fixture
from oracle import sa_oracle as so
from scrna_seq_qannealing_clustering_amd import graphs, models

WEIGHT_LIMIT = 1 << 30           # mi_sa_problem_set_node_weights: the largest total of the integer node weights
PATTERNS = ("degrees", "zeros", "hub", "tiny", "free_cw")

F8T, F8 = "k_anneal_potts_fast<16, 8, tw, weighted>", "k_anneal_potts_fast<16, 8, weighted>"
F16T, F16 = "k_anneal_potts_fast<16, 16, tw, weighted>", "k_anneal_potts_fast<16, 16, weighted>"
K3W = "k_anneal_potts<%d, weighted>"
KERNELS = (F8T, F8, F16T, F16, K3W % 16, K3W % 32, K3W % 64, K3W % 0)
NO_TW, NO_K3F = (("k2_tw", 2),), (("k3_fast", 2),)


@dataclasses.dataclass(frozen=True)
class Spec:
    """One row of the table: where the case's arrays come from."""
    name: str
    graph: str                   # key of GRAPHS
    order: Optional[str]         # Problem.potts_csr(order=)
    options: Tuple               # ((key, value), ...) for Problem.set_option
    K: int
    pattern: str                 # one of PATTERNS
    kernel: str                  # the anneal kernel the library plans for it
    R: int = 3
    picks: Tuple[int, ...] = (0, 1, 2)       # the replicas the restatement runs (all of them when R == len(picks))
    seed: int = 9
    hot: float = 0.3             # the schedule: np.geomspace(hot, cold, S) / (the median over the cells of sum_j |S_ij|)
    cold: float = 30.0
    S: int = 8
    replica_offset: int = 4


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    pattern: str
    rowptr: np.ndarray           # the model in the caller's order: CSR, fp64 couplings
    col: np.ndarray
    val: np.ndarray
    K: int
    wq: np.ndarray               # int32 weights, fp32 coefficients of the chain; fp64 weights, pair coefficient and
    cw: np.ndarray               # offset of the reported energies
    w64: np.ndarray
    c64: float
    offset: float
    order: Optional[str]
    options: Tuple
    betas: np.ndarray
    R: int
    picks: Tuple[int, ...]
    expected_kernel: str
    seed: int
    replica_offset: int
    hub: Optional[int]           # (pattern "hub": the heavy node, in the caller's order)

    @property
    def model(self):
        """The case as a PottsModel (what tests/test_gpu_modularity.py:problem and device_model take)."""
        n = len(self.rowptr) - 1
        lin = np.zeros(n, dtype=np.float64)
        lin[0] = self.offset
        return models.PottsModel([str(i) for i in range(n)], self.K, self.rowptr, self.col, self.val, c_pair=self.c64,
                                 lin=lin, info={"kind": "node_weight_case"}, node_weight=self.w64)

    @property
    def weights(self):
        return self.wq, self.cw, self.w64


def _s16():
    return graphs.EdgeListGraph(*graphs.synthetic_snn(640, 5, 15, 15, 6, seed=1, spread=3.0)[:4])


def _wide(n, max_deg):
    def make():
        from test_gpu_structured import wide_row_edges
        edges, w = wide_row_edges(n, max_deg)
        e = np.asarray(edges, dtype=np.int32)
        return graphs.EdgeListGraph([str(i) for i in range(n)], e[:, 0], e[:, 1], w.astype(np.float64))
    return make


GRAPHS = {
    "s16": _s16,                                             # tests/test_gpu_modularity.py:graph("s16"): no in-slot edges
    "noisy_circles": lambda: load_fixture("noisy_circles").graph(),
    "aniso": lambda: load_fixture("aniso").graph(),
    "blobs": lambda: load_fixture("blobs").graph(),
    "wide200": _wide(200, 100),                              # tests/test_gpu_structured.py:test_rows_wider_than_64
    "wide130": _wide(130, 129),                              # (the complete graph)
}
WIDE = {"wide200": 112, "wide130": 144}                      # their slot-ELL widths: the row width up to a multiple of 16
IN_SLOT = ("noisy_circles", "aniso", "blobs")                # golden graphs, too dense for slots free of internal edges

SPECS = [
    # ---- K3f, 8 label fields: with its threshold wavefront, and without
    Spec("f8tw_k3_degrees", "s16", "padded", (), 3, "degrees", F8T),
    Spec("f8tw_k8_zeros", "s16", "padded", (), 8, "zeros", F8T, R=6, picks=(1, 4)),
    Spec("f8tw_k3_hub", "s16", "padded", (), 3, "hub", F8T, R=6, picks=(0, 5)),
    Spec("f8tw_k8_tiny", "s16", "padded", (), 8, "tiny", F8T, R=6, picks=(2, 3)),
    Spec("f8_k8_tiny", "s16", "padded", NO_TW, 8, "tiny", F8),
    Spec("f8_k8_free_cw", "s16", "padded", NO_TW, 8, "free_cw", F8, R=6, picks=(0, 5)),
    Spec("f8_k3_zeros", "s16", "padded", NO_TW, 3, "zeros", F8, R=6, picks=(1, 4)),
    Spec("f8_k3_hub", "s16", "padded", NO_TW, 3, "hub", F8, R=6, picks=(2, 3)),
    Spec("f8_k8_degrees", "s16", "padded", NO_TW, 8, "degrees", F8, R=6, picks=(0, 5)),
    # ---- K3f, 16 label fields
    Spec("f16tw_k9_tiny", "s16", "padded", (), 9, "tiny", F16T),
    Spec("f16tw_k9_free_cw", "s16", "padded", (), 9, "free_cw", F16T, R=6, picks=(1, 4)),
    Spec("f16tw_k16_hub", "s16", "padded", (), 16, "hub", F16T, R=6, picks=(0, 5)),
    Spec("f16tw_k16_zeros", "s16", "padded", (), 16, "zeros", F16T, R=6, picks=(2, 3)),
    Spec("f16_k16_degrees", "s16", "padded", NO_TW, 16, "degrees", F16),
    Spec("f16_k16_zeros", "s16", "padded", NO_TW, 16, "zeros", F16, R=6, picks=(1, 4)),
    Spec("f16_k9_hub", "s16", "padded", NO_TW, 9, "hub", F16, R=6, picks=(0, 5)),
    Spec("f16_k9_degrees", "s16", "padded", NO_TW, 9, "degrees", F16, R=6, picks=(2, 3)),
    # ---- K3, D = 16: the s16 graph with K3f turned off, and with more labels than K3f takes
    Spec("d16_k17_degrees", "s16", "padded", NO_K3F, 17, "degrees", K3W % 16),
    Spec("d16_k32_zeros", "s16", "padded", NO_K3F, 32, "zeros", K3W % 16, R=6, picks=(1, 4)),
    Spec("d16_k33_hub", "s16", "padded", NO_K3F, 33, "hub", K3W % 16, R=6, picks=(0, 5)),
    Spec("d16_k64_tiny", "s16", "padded", NO_K3F, 64, "tiny", K3W % 16, R=6, picks=(2, 3)),
    Spec("d16_k17_free_cw", "s16", "padded", NO_K3F, 17, "free_cw", K3W % 16, R=6, picks=(0, 5)),
    Spec("d16_k8_hub", "s16", "padded", NO_K3F, 8, "hub", K3W % 16, R=6, picks=(1, 4)),
    # ---- K3, D = 32 and 64: golden graphs, edges inside the slots
    Spec("d32_k33_degrees", "noisy_circles", "padded", (), 33, "degrees", K3W % 32),
    Spec("d32_k64_hub", "noisy_circles", "padded", (), 64, "hub", K3W % 32, R=6, picks=(0, 3, 5)),
    Spec("d32_k32_zeros", "aniso", "slots", NO_K3F, 32, "zeros", K3W % 32, R=6, picks=(1, 2, 4)),
    Spec("d32_k17_tiny", "aniso", "slots", NO_K3F, 17, "tiny", K3W % 32, R=6, picks=(0, 3, 5)),
    Spec("d64_k33_free_cw", "blobs", "slots", (), 33, "free_cw", K3W % 64),
    # ---- K3, rows wider than 64: the runtime-width form
    Spec("wide200_k17_degrees", "wide200", None, (), 17, "degrees", K3W % 0),
    Spec("wide200_k64_zeros", "wide200", "slots", (), 64, "zeros", K3W % 0, R=6, picks=(0, 3, 5)),
    Spec("wide200_k32_free_cw", "wide200", None, (), 32, "free_cw", K3W % 0, R=6, picks=(1, 2, 4)),
    Spec("wide200_k33_tiny", "wide200", "slots", (), 33, "tiny", K3W % 0),
    Spec("wide130_k33_hub", "wide130", None, (), 33, "hub", K3W % 0),
    Spec("wide130_k64_tiny", "wide130", "slots", (), 64, "tiny", K3W % 0, R=6, picks=(0, 3, 5), hot=5.0, cold=200.0),
    Spec("wide200_k64_degrees", "wide200", None, (), 64, "degrees", K3W % 0, R=6, picks=(1, 2, 4)),
    Spec("wide130_k17_hub", "wide130", "slots", (), 17, "hub", K3W % 0, R=6, picks=(0, 3, 5)),
]
BY_NAME = {s.name: s for s in SPECS}
NAMES = [s.name for s in SPECS]
# the cases of the GPU test's further runs: a run continued in two pieces, and two resolution groups
CONTINUED = ("f16tw_k16_hub", "wide200_k64_zeros")
GROUPED = ("wide130_k33_hub", "d16_k33_hub")
GROUP_FACTOR = 1.6               # the second group: the first one's coefficients, constants and betas times this


@functools.lru_cache(maxsize=None)
def graph(name):
    return GRAPHS[name]()


def pattern_weights(pattern, pm, rs):
    """``(wq, cw, w64, c64, offset, hub)`` of a pattern on the modularity model ``pm``.  ``degrees`` is the model's own.
    The others keep its pair coefficient c = gamma / 2m and scale their integer weights to the same total 2m,
    ``w64 = wq 2m / sum wq``, so that the pair term stays of the size of the couplings: cw = fp32(c (2m / sum wq)^2 wq)."""
    n = pm.num_variables
    if pattern == "degrees":
        wq, cw, w64 = models.potts_node_weights(pm)
        return wq, cw, w64, float(pm.c_pair), pm.lin_offset, None
    hub = None
    if pattern == "zeros":
        wq = rs.randint(1, 1000, size=n)
        wq[rs.permutation(n)[:n // 3]] = 0
    elif pattern == "hub":
        hub = n // 2
        mean = (1 << 29) // (n - 1)
        wq = rs.randint(mean // 2, 3 * mean // 2, size=n)                 # small beside the hub, about 2^29 together
        wq[hub] = 0
        surplus = int(wq.sum()) - (1 << 29)
        others = np.flatnonzero(np.arange(n) != hub)
        wq[others] -= surplus // (n - 1)
        wq[others[:surplus % (n - 1)]] -= 1
        wq[hub] = 1 << 29
        assert wq.min() > 0 and int(wq.sum()) == WEIGHT_LIMIT
    elif pattern == "tiny":
        wq = rs.randint(0, 3, size=n)
    elif pattern == "free_cw":
        wq = rs.randint(1, 1001, size=n)
    else:
        raise ValueError(pattern)
    wq = wq.astype(np.int32)
    two_m = 2.0 * pm.info["m"]
    scale = two_m / float(wq.sum())
    c64 = float(pm.c_pair)
    w64 = scale * wq.astype(np.float64)
    basis = rs.randint(1, 1001, size=n) if pattern == "free_cw" else wq            # (free_cw: not the weights)
    cw = (c64 * scale * scale * basis.astype(np.float64)).astype(np.float32)
    offset = c64 * float(np.sum(w64 * w64)) / 2.0
    return wq, cw, w64, c64, offset, hub


@functools.lru_cache(maxsize=None)
def case(name):
    s = BY_NAME[name]
    pm = models.build_modularity_potts(graph(s.graph), 1.0, s.K)
    rs = np.random.RandomState(s.seed + 1000 * PATTERNS.index(s.pattern))
    wq, cw, w64, c64, offset, hub = pattern_weights(s.pattern, pm, rs)
    rows = np.repeat(np.arange(pm.num_variables), np.diff(pm.rowptr))
    field = np.zeros(pm.num_variables)
    np.add.at(field, rows, np.abs(pm.val))
    betas = np.geomspace(s.hot, s.cold, s.S) / float(np.median(field[field > 0]))
    for arr in (wq, cw, w64, betas):
        arr.setflags(write=False)
    return Case(name, s.pattern, pm.rowptr, pm.col, pm.val, s.K, wq, cw, w64, c64, offset, s.order, s.options, betas, s.R,
                s.picks, s.kernel, s.seed, s.replica_offset, hub)


def cases():
    """Every case of the table by name."""
    return {name: case(name) for name in NAMES}


@dataclasses.dataclass(frozen=True)
class DeviceInputs:
    """A case as the device sweeps it (padded / permuted seats, holes)."""
    rowptr: np.ndarray
    col: np.ndarray
    val: np.ndarray              # fp32
    wq: np.ndarray               # int64, 0 at the holes
    cw: np.ndarray               # fp32
    absent: np.ndarray
    seats: np.ndarray            # seat of each of the caller's variables
    val64: np.ndarray
    w64: np.ndarray

    def arrays(self):
        return tuple(getattr(self, f.name) for f in dataclasses.fields(self))


def device_inputs(layout, c, cw=None):
    """``layout``: an engine.Problem or a potts_merge_cases.Layout (``_inv``, ``n_dev``).  ``cw``: other coefficients than
    the case's (a resolution group's)."""
    from test_gpu_modularity import device_model
    pm = c.model
    rp, cc, vv, dq, dc, absent, seats = device_model(layout, pm, c.wq, c.cw if cw is None else cw)
    val64 = models.pad_csr(pm.rowptr, pm.col, pm.val, seats, layout.n_dev)[2].astype(np.float64)
    dw = np.zeros(layout.n_dev, dtype=np.float64)
    dw[seats] = c.w64
    return DeviceInputs(rp, cc, vv, dq, dc, absent, np.asarray(seats), val64, dw)


@functools.lru_cache(maxsize=None)
def inputs(name):
    from potts_merge_cases import Layout
    c = case(name)
    d = device_inputs(Layout(c.model, c.order), c)
    for arr in d.arrays():
        arr.setflags(write=False)
    return d


def slot_ell_width(rowptr):
    """The library's slot-ELL width D for rows of this CSR (csrc/mi_sa.hip): 16, 32, 64, or the next multiple of 16."""
    w = int(np.diff(rowptr).max())
    return 16 if w <= 16 else 32 if w <= 32 else 64 if w <= 64 else (w + 15) // 16 * 16


def chain2d_frozen_sums(d, K, betas, seed, replica_offset, replicas):
    """Chain 2d as a WRONG kernel would run it: every lane of a 64-seat slot evaluated against the cluster sums from the start
    of the slot, the movers below it ignored (the sums themselves are kept up to date, so the next slot starts right).
    ``d``: DeviceInputs -- the seats are the order the device sweeps.  A local copy of chain2d's loop with that one change;
    a case on which it ends where chain2d does could not tell the two apart.  Returns the labels [len(replicas), n_dev]."""
    from test_modularity_model import fmaf
    rowptr, col, wq, cw = d.rowptr.astype(np.int64), d.col.astype(np.int64), d.wq, d.cw
    n = len(rowptr) - 1
    temps = [np.float32(1.0 / b) for b in np.asarray(betas, dtype=np.float64)]
    rows = [(col[rowptr[i]:rowptr[i + 1]].tolist(), d.val[rowptr[i]:rowptr[i + 1]].tolist()) for i in range(n)]
    out = np.zeros((len(replicas), n), dtype=np.uint16)
    for k, r in enumerate(replicas):
        gid = replica_offset + r
        lab = [0 if d.absent[i] else so.chain_word(seed, i, 0, gid, 1) % K for i in range(n)]
        W = [0] * K
        for i in range(n):
            if not d.absent[i]:
                W[lab[i]] += int(wq[i])
        for s, T in enumerate(temps):
            for i in range(n):
                if i % 64 == 0:
                    Wf = list(W)                             # <-- the sums every lane of this slot reads
                if d.absent[i]:
                    continue
                a = lab[i]
                b = (a + 1 + so.chain_word(seed, i, s, gid, 2) % (K - 1)) % K
                hd = np.float32(0.0)
                for j, v in zip(*rows[i]):
                    lj = lab[j]
                    if lj == b:
                        hd = np.float32(hd + np.float32(v))
                    elif lj == a:
                        hd = np.float32(hd - np.float32(v))
                dE = fmaf(cw[i], np.float32(Wf[b] - Wf[a] + int(wq[i])), hd)
                if dE < np.float32(so.neglog_u(so.chain_word(seed, i, s, gid, 0))) * T:
                    lab[i] = b
                    W[a] -= int(wq[i])
                    W[b] += int(wq[i])
        out[k] = lab
    return out


@dataclasses.dataclass(frozen=True)
class Reference:
    labels: np.ndarray           # [len(picks), n_dev]
    accepted: int                # over the picked replicas
    energies: np.ndarray         # fp64, as the device reports them
    accepts: np.ndarray          # [S]: accepted moves per sweep
    rejects: np.ndarray          # [S]
    d_values: np.ndarray         # the distinct W_b - W_a + wq_i the run evaluated
    hub_accepts: int             # accepted moves of the hub (pattern "hub")
    seconds: float


@functools.lru_cache(maxsize=None)
def reference(name):
    """chain2d's run of a case on its picked replicas, once per session and left unchanged."""
    from test_modularity_model import chain2d
    c, d = case(name), inputs(name)
    trace = []
    t0 = time.perf_counter()
    lab, acc, en = chain2d(d.rowptr, d.col, d.val, d.wq, d.cw, c.K, c.R, c.betas, c.seed, replica_offset=c.replica_offset,
                           absent=d.absent, replicas=list(c.picks), energy=(d.val64, d.w64, c.c64, c.offset), trace=trace)
    dt = time.perf_counter() - t0
    S = len(c.betas)
    sweep = np.array([t[1] for t in trace])
    ok = np.array([t[4] for t in trace])
    hub_seat = -1 if c.hub is None else int(d.seats[c.hub])
    hub_accepts = sum(1 for t in trace if t[2] == hub_seat and t[4])
    dv = np.unique(np.array([t[3] for t in trace], dtype=np.int64))
    for arr in (lab, en):
        arr.setflags(write=False)
    return Reference(lab, acc, en, np.bincount(sweep[ok], minlength=S), np.bincount(sweep[~ok], minlength=S), dv,
                     hub_accepts, dt)


@functools.lru_cache(maxsize=None)
def frozen_labels(name):
    c = case(name)
    return chain2d_frozen_sums(inputs(name), c.K, c.betas, c.seed, c.replica_offset, list(c.picks))


def second_group(c):
    """The second resolution group of the GPU test's grouped runs: ``(cw, c64, offset, betas)``."""
    f = GROUP_FACTOR
    return (f * c.cw.astype(np.float64)).astype(np.float32), f * c.c64, f * c.offset, c.betas / f
