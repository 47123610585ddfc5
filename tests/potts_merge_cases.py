"""The edge cases of the Potts merge phase (chain 2e, k_potts_merge) shared by tests/test_potts_merge_cases.py, which shows
on the CPU that the restatement really merges where each case is meant to reach, and tests/test_gpu_potts_merge_edges.py,
which holds the device to the restatement on them.  TEST INFRASTRUCTURE ONLY.

Every case runs the restatement (tests/test_potts_merge_model.py:chain2e, with its trace) once per session on the model as
the device sweeps it; the seats of that layout are computed here without a GPU (``Layout``) and the GPU test checks that
the problem it creates took the same ones."""
import dataclasses
import functools
import time
from typing import Optional, Tuple

import numpy as np

from scrna_seq_qannealing_clustering_amd import graphs, models
from scrna_seq_qannealing_clustering_amd.sampler import default_potts_beta_range

WEIGHT_LIMIT = 1 << 30           # mi_sa_problem_set_node_weights: the largest total of the integer node weights


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    graph: str                   # key of GRAPHS
    kind: str                    # "mod" (modularity, node weights) / "dqm" (unweighted, cq = c_pair) / "heavy" (mod, sum wq = 2^30)
    K: int
    R: int                       # replicas (per resolution group)
    M: int                       # merge interval
    P: int                       # proposals per merge phase
    S: int                       # sweeps
    sched: Tuple                 # ("hot", f): (f lo, hi) of default_potts_beta_range; ("abs", b0, b1): as given
    seed: int
    kernel: str                  # the anneal kernel the library plans for it (read from the device once, then fixed here)
    gammas: Tuple[float, ...] = (1.0,)      # more than one: resolution groups, R replicas each
    order: Optional[str] = "padded"
    per_replica: bool = False    # one constant beta per replica (geometric over the schedule's range)
    replica_offset: int = 5
    sweep_offset: int = 0
    starts: Tuple = (None,)      # None: the chain's tag-1 words; "all": caller's labels using every value; "two": only {5, 63}


def _snn(n, k=5, o=15, clusters=6, seed=1):
    return lambda: graphs.EdgeListGraph(*graphs.synthetic_snn(n, k, 15, o, clusters, seed=seed, spread=3.0)[:4])


def _wide():
    from test_gpu_structured import wide_row_edges
    edges, w = wide_row_edges(130, 129)
    e = np.asarray(edges, dtype=np.int32)
    return graphs.EdgeListGraph([str(i) for i in range(130)], e[:, 0], e[:, 1], w.astype(np.float64))


GRAPHS = {
    "snn150": _snn(150),
    "snn20": _snn(20, clusters=3),
    "pair": lambda: graphs.EdgeListGraph(["0", "1"], [0], [1], [1.0]),
    "snn63": _snn(63), "snn64": _snn(64), "snn65": _snn(65), "snn257": _snn(257),
    "isolated40": lambda: graphs.EdgeListGraph([str(i) for i in range(40)], np.zeros(0, np.int32), np.zeros(0, np.int32),
                                               np.zeros(0)),
    "wide130": _wide,
    "dense130": _snn(130, k=8, o=30),                       # too dense for ceil(n / 64) slots: holes between the cells
}

HOT4 = ("hot", 4.0)              # the schedule of tests/test_gpu_potts_merge.py: merges are accepted on it
K3W, K3 = "k_anneal_potts<%d, weighted>", "k_anneal_potts<%d>"
K3F = "k_anneal_potts_fast<%d, %d, tw, weighted>"

CASES = [
    Case("p_two_passes", "snn150", "mod", 64, 8, 3, 130, 6, HOT4, 29, K3W % 16),
    Case("p_65", "snn150", "mod", 33, 8, 1, 65, 6, HOT4, 29, K3W % 16),
    Case("p_64", "snn150", "mod", 32, 4, 1, 64, 6, HOT4, 28, K3W % 16),
    Case("p_1", "snn150", "mod", 8, 8, 1, 1, 6, HOT4, 29, K3F % (16, 8)),
    Case("k_2_mod", "snn150", "mod", 2, 4, 1, 3, 4, ("abs", 0.02, 0.2), 29, K3F % (16, 8)),
    Case("k_2_dqm", "snn150", "dqm", 2, 4, 1, 3, 4, ("abs", 0.02, 0.2), 29, "k_anneal_potts_fast<16, 8, tw>"),
    Case("k_63", "snn150", "mod", 63, 2, 2, 126, 6, HOT4, 29, K3W % 16),
    Case("k_64_dqm", "snn150", "dqm", 64, 2, 2, 131, 6, HOT4, 29, K3 % 16),
    Case("k_above_n", "snn20", "mod", 64, 4, 2, 128, 6, HOT4, 29, K3W % 16),
    # device n = the caller's n (order=None: no padding), so the i < n tails of (a) and (c) and the last partial slot run
    Case("ragged_n2", "pair", "mod", 12, 8, 1, 27, 4, HOT4, 29, K3W % 16, order=None),
    Case("ragged_n63", "snn63", "mod", 12, 2, 2, 27, 6, HOT4, 29, K3W % 16, order=None),
    Case("ragged_n64", "snn64", "mod", 12, 2, 2, 27, 6, HOT4, 29, K3W % 16, order=None),
    Case("ragged_n65", "snn65", "mod", 12, 2, 2, 27, 6, HOT4, 29, K3W % 16, order=None),
    Case("ragged_n65_dqm", "snn65", "dqm", 12, 2, 2, 27, 6, HOT4, 29, K3 % 16, order="slots"),
    Case("ragged_n257", "snn257", "mod", 12, 2, 2, 27, 6, HOT4, 29, K3W % 16, order=None),
    # ... and the padded layouts of the same sizes (device n a multiple of 64, holes): two slots for two cells, ten for 257
    Case("padded_n2", "pair", "mod", 12, 8, 1, 27, 4, HOT4, 29, K3F % (16, 16)),
    Case("padded_n257", "snn257", "mod", 12, 2, 2, 27, 6, HOT4, 29, K3F % (16, 16)),
    Case("no_couplings", "isolated40", "dqm", 8, 4, 2, 19, 6, ("abs", 0.5, 4.0), 29, "k_anneal_potts_fast<16, 8, tw>"),
    Case("wide_rows_k15", "wide130", "mod", 15, 2, 2, 33, 6, HOT4, 29, K3W % 0),
    Case("wide_rows_k40", "wide130", "dqm", 40, 2, 2, 83, 6, HOT4, 29, K3 % 0, order="slots"),
    Case("holes", "dense130", "mod", 12, 2, 2, 27, 6, HOT4, 29, K3W % 32),
    Case("heavy_weights", "snn150", "heavy", 8, 4, 2, 19, 6, HOT4, 29, K3F % (16, 8)),
    Case("groups_k64", "snn150", "mod", 40, 5, 2, 90, 5, HOT4, 41, K3W % 16, gammas=(0.5, 1.0, 1.6), replica_offset=2),
    Case("per_replica_k64", "snn150", "mod", 64, 7, 2, 130, 4, HOT4, 29, K3W % 16, per_replica=True),
    Case("opens_with_merge_k64", "snn150", "mod", 64, 8, 4, 200, 1, HOT4, 24, K3W % 16, sweep_offset=4, replica_offset=0,
         starts=(None, "all", "two")),
    # two clusters hold every cell: 2 of the 4032 ordered pairs can merge, so many passes for most replicas to meet one
    Case("opens_two_labels_k64", "snn150", "mod", 64, 16, 4, 4096, 1, ("hot", 1.0), 24, K3W % 16, sweep_offset=4, replica_offset=0,
         starts=("two",)),
]
BY_NAME = {c.name: c for c in CASES}
# the n the device gets (mi_sa's p->n, MergeArgs.n) where a case is about it
DEVICE_N = {"ragged_n2": 2, "ragged_n63": 63, "ragged_n64": 64, "ragged_n65": 65, "ragged_n65_dqm": 65, "ragged_n257": 257,
            "padded_n2": 128, "padded_n257": 640, "wide_rows_k40": 130}
RUNS = [(c.name, g, st) for c in CASES for g in range(len(c.gammas)) for st in c.starts]     # one restatement run each


def run_id(run):
    name, g, st = run
    return name + ("-g%d" % g if len(BY_NAME[name].gammas) > 1 else "") + ("-%s" % st if st else "")


@functools.lru_cache(maxsize=None)
def graph(name):
    return GRAPHS[name]()


def heavy_model(pm):
    """``pm`` with its node weights rescaled so that the quantised ones sum to exactly WEIGHT_LIMIT (the most the ABI admits):
    the products W_a W_b of the merge phase then pass 2^53 and are rounded on their way to fp64."""
    wq, _, _ = models.potts_node_weights(pm)
    e = pm.info["scale_exp"]
    big = (wq.astype(np.int64) * WEIGHT_LIMIT) // int(wq.sum())
    big[:WEIGHT_LIMIT - int(big.sum())] += 1                                  # the remainder, one unit each
    heavy = dataclasses.replace(pm, node_weight=np.ldexp(big.astype(np.float64), -e))
    got, _, e2 = models.quantise_node_weights(heavy.node_weight, heavy.c_pair)
    assert e2 == e and np.array_equal(got, big) and int(got.sum()) == WEIGHT_LIMIT
    return heavy


@functools.lru_cache(maxsize=None)
def model(name, g=0):
    """The Potts model of a case (of its resolution group ``g``)."""
    c = BY_NAME[name]
    G = graph(c.graph)
    if c.kind == "dqm":
        return models.build_dqm_potts(G, c.K, 0.005)
    pm = models.build_modularity_potts(G, c.gammas[g], c.K)
    return heavy_model(pm) if c.kind == "heavy" else pm


def beta_range(c, pm):
    if c.sched[0] == "abs":
        return c.sched[1], c.sched[2]
    lo, hi = default_potts_beta_range(pm)
    return c.sched[1] * lo, hi


def betas(c, pm):
    """The schedule of one group: [S] betas, and the per-replica betas (or None)."""
    rng = beta_range(c, pm)
    return models.make_beta_schedule(c.S, rng), (np.geomspace(rng[0], rng[1], c.R) if c.per_replica else None)


def start_labels(c, st):
    """The caller's labels of a start: [R, n] uint16 in the caller's variable order, or None (tag-1 words)."""
    if st is None:
        return None
    n = model(c.name).num_variables
    rs = np.random.RandomState(3)
    if st == "all":
        assert n >= c.K
        lab = np.stack([rs.permutation(n) % c.K for _ in range(c.R)])
        assert all(len(np.unique(row)) == c.K for row in lab)
    else:
        lab = rs.choice([5, 63], size=(c.R, n))
    return lab.astype(np.uint16)


class Layout:
    """The seats Problem.potts_csr gives a model's variables, without a GPU: what tests/test_gpu_modularity.py:device_model
    reads of a problem (``_inv``, ``n_dev``)."""

    def __init__(self, pm, order):
        n = pm.num_variables
        self._inv, self.n_dev = None, n
        if order == "padded":
            seats, nslots, _ = models.padded_slot_layout(pm.rowptr, pm.col)
            self._inv, self.n_dev = np.asarray(seats, dtype=np.int64), nslots * 64
        elif order == "slots":
            self._inv = np.argsort(models.slot_independent_order(pm.rowptr, pm.col))


@dataclasses.dataclass(frozen=True)
class Reference:
    inputs: Tuple                # chain_inputs(...): (rowptr, col, val, wq, cw, cq, absent, seats) in device seats
    labels: np.ndarray           # [R, n_dev]
    accepted: int                # single-site moves
    merges: int
    trace: Tuple                 # (kind, replica, sweep, p, a, b, W_a W_b) per proposal, kind "accept" / "empty" / "reject"
    seconds: float


@functools.lru_cache(maxsize=None)
def reference(run):
    """The restatement's run of ``run = (case, group, start)``, once per session and left unchanged."""
    from test_gpu_potts_merge import chain_inputs
    from test_potts_merge_model import chain2e
    name, g, st = run
    c = BY_NAME[name]
    pm = model(name, g)
    rp, cc, vv, dq, dc, cq, absent, seats = inputs = chain_inputs(Layout(pm, c.order), pm)
    sched, rb = betas(c, pm)
    start = start_labels(c, st)
    dinit = None
    if start is not None:
        dinit = np.zeros((c.R, len(rp) - 1), dtype=np.uint16)
        dinit[:, seats] = start
    trace = []
    t0 = time.perf_counter()
    olab, oacc, omerges = chain2e(rp, cc, vv, dq, dc, cq, c.K, c.R, sched, c.seed, c.M, c.P,
                                  replica_offset=c.replica_offset, init=dinit, sweep_offset=c.sweep_offset, absent=absent,
                                  per_replica=rb, trace=trace)
    dt = time.perf_counter() - t0
    for arr in inputs:
        if isinstance(arr, np.ndarray):
            arr.setflags(write=False)
    olab.setflags(write=False)
    return Reference(inputs, olab, oacc, omerges, tuple(trace), dt)
