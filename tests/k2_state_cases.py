"""The cases that run EVERY form of K2 (k_anneal_csr_rank1<D, XS, TW>, csrc/sparse_kernels.hip) at sizes where the C oracle
costs milliseconds, shared by tests/test_k2_state_cases.py -- which shows without a GPU that each case plans to the kernel
it names and is not vacuous on the oracle alone -- and tests/test_gpu_k2_state_forms.py, which holds the device to the
oracle on them.  TEST INFRASTRUCTURE ONLY.

K2 is built in 16 forms: the slot-ELL width D = 16 / 32 / 64 / 0 (0: the runtime width, rows wider than 64) times the
state in LDS, a half (XS = 2), a byte (1) or a bit (0) per variable, plus the four forms with a threshold wavefront
(``tw``: bit and byte state at D = 16 / 32).  The library keeps the half form up to 4608 variables; ``MI_K2_STATE`` = byte |
bit, read when a model is created, narrows the state at any size, which is how the byte and bit forms run here.

A case is a model x a state form x (threshold wavefront or not) x a scenario, and names its kernel.  The models (MODELS)
take the sizes 1, 31, 33, 63, 64, 65, 130, 257, 700 (1, 2, 3, 5 and 11 slots: a partial group of four slots, a whole group
plus one, two groups plus three), maximum degrees 3 .. 129 (every D, W = 80 and 144 in the runtime-width form), models
swept in the caller's order with up to 12 neighbours of a variable inside its own slot (the ``rows[]`` tail of the kernel's
serial loop takes over at the fifth), renumbered (``slots``) and padded ones (holes, the integer fast path), one whose slots
are partly flagged, and one with pair-term weights.  SCENARIOS lists what a run can be.  Every model is forced onto K2 by
``k2_pair`` = 2 and ``k2_split`` = 2; ``k2_tw`` = 2 turns the threshold wavefront off, as does a run of more than 1024
replicas (scenario ``many``)."""
import dataclasses
import functools
from typing import Optional, Tuple

import numpy as np

from oracle import sa_oracle as so
from scrna_seq_qannealing_clustering_amd import engine, models

SCENARIOS = ("random", "init", "offset", "resync", "split", "perbeta", "weighted", "energy64", "many")
STATES = (None, "byte", "bit")                   # MI_K2_STATE of the case (None: unset, the half form at these sizes)
XS = {None: 2, "byte": 1, "bit": 0}
VALUES = np.array([1 / 9, 0.25, 3 / 7, 2 / 3, 1.0, -0.5])      # the couplings, as tests/test_gpu_structured.py draws them
MANY_R, MANY_PICKS, MANY_WIDTH = 1100, (0, 548, 1096), 4       # scenario "many": the oracle on three slices of four replicas


def K(D, xs, tw=False):
    return "k_anneal_csr_rank1<%d, %d%s>" % (D, xs, ", tw" if tw else "")


ALL_KERNELS = tuple(K(D, xs) for D in (16, 32, 64, 0) for xs in (2, 1, 0)) + tuple(
    K(D, xs, True) for D in (16, 32) for xs in (1, 0))
assert len(set(ALL_KERNELS)) == 16


# ---- the models ----------------------------------------------------------------------------------------------------------
def _ring(n, offsets):
    return sorted({(min(i, (i + d) % n), max(i, (i + d) % n)) for i in range(n) for d in offsets if (i + d) % n != i})


def _mixed(n=257):
    """Every variable tied to i + 64 and i + 128 (mod n: always another slot); slots 0 and 2 also carry a ring of offsets
    1 .. 6 inside themselves.  Slots 0 and 2 take the kernel's serial loop, slots 1, 3 and 4 its integer fast path."""
    pairs = set(_ring(n, (64, 128)))
    for t in (0, 2):
        for i in range(64 * t, 64 * t + 64):
            for d in range(1, 7):
                if i + d < 64 * t + 64:
                    pairs.add((i, i + d))
    return sorted(pairs)


def _capped(n, max_deg):
    def make():
        from test_gpu_structured import wide_row_edges              # a few hubs at the cap and a sparse rest / the complete graph
        return [(int(a), int(b)) for a, b in wide_row_edges(n, max_deg)[0]]
    return make


@dataclasses.dataclass(frozen=True)
class ModelSpec:
    n: int
    edges: object                # a callable -> sorted list of (lo, hi)
    order: Optional[str]         # Problem.csr_rank1(order=)
    c_pair: float
    D: int                       # the template width of the device rows (0: the runtime-width form)
    W: int                       # ... and the stored row width
    heavy: int = 0               # variables with pair-term weights other than 1, behind the n coupled ones
    hot: float = 0.05            # betas = np.geomspace(hot, cold, sweeps)
    cold: float = 4.0


RING6 = (1, 2, 3, 4, 5, 6)
MODELS = {
    "n1": ModelSpec(1, lambda: [], None, 0.4, 16, 16),
    "ring31": ModelSpec(31, lambda: _ring(31, RING6), None, 0.03, 16, 16),           # bit form: one 32-bit state word
    "ring33": ModelSpec(33, lambda: _ring(33, RING6), None, -0.02, 16, 16),          # ... and two
    "ring63": ModelSpec(63, lambda: _ring(63, RING6), None, 0.0, 16, 16),
    "ring64": ModelSpec(64, lambda: _ring(64, RING6), None, 0.4, 16, 16),
    "ring65": ModelSpec(65, lambda: _ring(65, RING6), None, 0.03, 16, 16),
    "ring130": ModelSpec(130, lambda: _ring(130, RING6 + (64,)), None, -0.02, 16, 16),
    "mixed257": ModelSpec(257, _mixed, None, 0.01, 16, 16),
    "deg3_700": ModelSpec(700, _capped(700, 3), "slots", 0.004, 16, 16),
    "deg16_257": ModelSpec(257, _capped(257, 16), "padded", -0.005, 16, 16),
    "deg17_257": ModelSpec(257, _capped(257, 17), None, 0.03, 32, 32),
    "deg30_700": ModelSpec(700, _capped(700, 30), "padded", 0.0, 32, 32),
    "deg32_700": ModelSpec(700, _capped(700, 32), None, 0.01, 32, 32),
    "deg33_130": ModelSpec(130, _capped(130, 33), None, 0.03, 64, 64),
    "deg64_257": ModelSpec(257, _capped(257, 64), None, -0.005, 64, 64),
    "deg70_257": ModelSpec(257, _capped(257, 70), None, 0.03, 0, 80),
    "complete130": ModelSpec(130, _capped(130, 129), None, 0.03, 0, 144, hot=0.01, cold=0.5),
    "weighted137": ModelSpec(130, _capped(130, 9), "padded", 0.03, 16, 16, heavy=7),
}
HEAVY_WEIGHTS = np.array([2, 4, 8, 16, 3, 5, 32])
# swept in the caller's order, with variables that have more than four neighbours inside their own slot
IN_SLOT = ("ring31", "ring33", "ring63", "ring64", "ring65", "ring130", "mixed257", "deg17_257", "deg32_700", "deg33_130",
           "deg64_257", "deg70_257", "complete130")


@dataclasses.dataclass(frozen=True)
class Model:
    """A model in the caller's order: fp64 coefficients (the energy model) and the fp32 ones the chain runs on."""
    name: str
    n: int
    rowptr: np.ndarray
    col: np.ndarray
    val64: np.ndarray
    lin64: np.ndarray
    c64: float
    val: np.ndarray
    lin: np.ndarray
    c_pair: float
    weights: Optional[np.ndarray]
    order: Optional[str]


@functools.lru_cache(maxsize=None)
def model(name):
    s = MODELS[name]
    rs = np.random.RandomState(4000 + list(MODELS).index(name))
    edges = s.edges()
    w = rs.choice(VALUES, size=len(edges))
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    rowptr, col, val64 = models._csr_from_edges(s.n, e[:, 0], e[:, 1], w)
    lin64 = rs.normal(scale=0.7, size=s.n)
    weights = None
    n = s.n
    if s.heavy:                  # slack-like variables: no couplings, a pair-term weight, small linear terms of both signs
        n = s.n + s.heavy
        rowptr = np.concatenate([rowptr, [rowptr[-1]] * s.heavy]).astype(np.int32)
        lin64 = np.concatenate([lin64, rs.normal(scale=0.3, size=s.heavy)])
        weights = np.concatenate([np.ones(s.n, dtype=np.int64), HEAVY_WEIGHTS[:s.heavy]])
    out = Model(name, n, rowptr.astype(np.int32), col.astype(np.int32), val64, lin64, float(s.c_pair),
                val64.astype(np.float32), lin64.astype(np.float32), float(np.float32(s.c_pair)), weights, s.order)
    for f in dataclasses.fields(out):
        if isinstance(getattr(out, f.name), np.ndarray):
            getattr(out, f.name).setflags(write=False)
    return out


@dataclasses.dataclass(frozen=True)
class DeviceModel:
    """The model as the device sweeps it: renumbered (``slots``) or seated with holes (``padded``, lin = +inf at a hole)."""
    n_dev: int
    rowptr: np.ndarray
    col: np.ndarray
    val: np.ndarray
    lin: np.ndarray
    weights: Optional[np.ndarray]            # int32 [n_dev] (1 at the holes), None: unweighted
    wslot: int                               # the slot of the weighted variables (-1: none)
    seats: np.ndarray                        # device column of the caller's variable i
    holes: np.ndarray
    val64: np.ndarray
    lin64: np.ndarray
    heavy: np.ndarray                        # device variables with more than four neighbours inside their own slot


@functools.lru_cache(maxsize=None)
def device_model(name):
    m = model(name)
    wdev, wslot = None, -1
    if m.weights is not None:
        rp, cc, vv, lin, wdev, seats, n_dev, val64, lin64 = engine.weighted_layout_csr(
            m.rowptr, m.col, m.val, m.lin, m.weights, energy_model=(m.val64, m.lin64, m.c64))
        slots = np.unique(np.flatnonzero(wdev != 1) // 64)
        assert len(slots) == 1
        wslot = int(slots[0])
    elif m.order == "slots":
        perm = models.slot_independent_order(m.rowptr, m.col)
        rp, cc, vv, val64 = models.permute_csr(m.rowptr, m.col, m.val, perm, also=m.val64)
        lin, lin64, seats, n_dev = m.lin[perm], m.lin64[perm], np.argsort(perm), m.n
    elif m.order == "padded":
        seats, nslots, clashes = models.padded_slot_layout(m.rowptr, m.col)
        assert clashes == 0
        n_dev = nslots * 64
        rp, cc, vv, val64 = models.pad_csr(m.rowptr, m.col, m.val, seats, n_dev, also=m.val64)
        lin = np.full(n_dev, np.inf, dtype=np.float32)
        lin[seats] = m.lin
        lin64 = np.zeros(n_dev)
        lin64[seats] = m.lin64
    else:
        rp, cc, vv, val64, lin, lin64, seats, n_dev = m.rowptr, m.col, m.val, m.val64, m.lin, m.lin64, np.arange(m.n), m.n
    rp, cc = np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(cc, dtype=np.int32)
    rows = np.repeat(np.arange(n_dev), np.diff(rp))
    inside = np.bincount(rows[(rows >> 6) == (cc >> 6)], minlength=n_dev)
    out = DeviceModel(int(n_dev), rp, cc, np.ascontiguousarray(vv, dtype=np.float32), np.ascontiguousarray(lin, dtype=np.float32),
                      wdev, wslot, np.asarray(seats, dtype=np.int64), np.setdiff1d(np.arange(n_dev), seats),
                      np.asarray(val64, dtype=np.float64), np.asarray(lin64, dtype=np.float64), np.flatnonzero(inside > 4))
    for f in dataclasses.fields(out):
        if isinstance(getattr(out, f.name), np.ndarray):
            getattr(out, f.name).setflags(write=False)
    return out


def energies64(name, X):
    """The fp64 host sum of the caller's model on states [R, n] (caller's order): lin . x + sum_{i<j} S_ij x_i x_j +
    c sum_{i<j} w_i w_j x_i x_j."""
    m = model(name)
    X = np.asarray(X, dtype=np.float64)
    rows = np.repeat(np.arange(m.n), np.diff(m.rowptr))
    w = np.ones(m.n) if m.weights is None else m.weights.astype(np.float64)
    s1, s2 = X @ w, X @ (w * w)
    return X @ m.lin64 + 0.5 * (X[:, rows] * X[:, m.col] * m.val64[None, :]).sum(axis=1) + m.c64 * 0.5 * (s1 * s1 - s2)


# ---- the cases -------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    model: str
    state: Optional[str]         # MI_K2_STATE
    tw: bool                     # beside a threshold wavefront
    scenario: str
    kernel: str                  # the name Problem.kernel_name() must report
    R: int = 5
    sweeps: int = 6

    @property
    def seed(self):
        return 50 + list(MODELS).index(self.model)                  # (one seed per model: its state forms run the same chain)

    @property
    def options(self) -> Tuple:
        off = (("k2_tw", 2),) if not self.tw and self.scenario != "many" and self.state is not None else ()
        return (("k2_pair", 2), ("k2_split", 2)) + off

    @property
    def betas(self):
        s = MODELS[self.model]
        if self.scenario == "perbeta":                              # one constant temperature per replica
            return np.geomspace(4 * s.hot, s.cold, self.R)
        return np.geomspace(s.hot, s.cold, self.sweeps)

    @property
    def init(self):
        """Given initial states in the caller's order (scenario ``init``)."""
        if self.scenario != "init":
            return None
        return np.random.RandomState(self.seed).randint(0, 2, size=(self.R, model(self.model).n)).astype(np.uint8)

    @property
    def run(self):
        """What the scenario adds to an anneal call / an oracle run (the same keywords but for the initial states)."""
        return {"offset": dict(replica_offset=2 ** 31 - 3), "resync": dict(resync_interval=2),
                "weighted": dict(replica_offset=2), "perbeta": dict(num_sweeps=self.sweeps, sweep_offset=100)}.get(self.scenario, {})


def make_case(model_name, state, tw, scenario, **kw):
    s = MODELS[model_name]
    assert not tw or (s.D in (16, 32) and state is not None)
    name = "%s-%s%s-%s" % (model_name, state or "half", "-tw" if tw else "", scenario)
    return Case(name, model_name, state, tw, scenario, K(s.D, XS[state], tw), **kw)


def _table():
    out = []
    # every model on the byte and the bit form from a random start -- beside a threshold wavefront where one is built
    for m, s in MODELS.items():
        if m == "weighted137":
            continue
        for state in ("byte", "bit"):
            out.append(make_case(m, state, s.D in (16, 32), "random", R=9 if m == "n1" else 5))
    # every scenario on both forms, with and without a threshold wavefront: (model beside one, model without)
    per_scenario = {
        "random": (None, "ring130"),                                # (with: the block above)
        "init": ("ring65", "deg17_257"),
        "offset": ("deg32_700", "ring33"),
        "resync": ("deg16_257", "mixed257"),
        "split": ("mixed257", "deg30_700"),
        "perbeta": ("deg17_257", "deg3_700"),
        "weighted": ("weighted137", "weighted137"),
        "energy64": ("deg30_700", "ring65"),
    }
    for scenario, (with_tw, without) in per_scenario.items():
        for state in ("byte", "bit"):
            if with_tw:
                out.append(make_case(with_tw, state, True, scenario, R=6))
            out.append(make_case(without, state, False, scenario, R=6))
    # the widths without a threshold wavefront, D = 64 and the runtime width: the scenarios that read or write the state
    # another way (given states, a continued run, the fp64 epilogue, holes do not occur at these widths)
    out += [make_case("deg33_130", "byte", False, "init"), make_case("deg33_130", "bit", False, "split"),
            make_case("deg64_257", "byte", False, "energy64"), make_case("deg64_257", "bit", False, "perbeta"),
            make_case("deg70_257", "byte", False, "split"), make_case("deg70_257", "bit", False, "init"),
            make_case("complete130", "byte", False, "perbeta"), make_case("complete130", "bit", False, "energy64")]
    # the half form of every width (what every model of this size runs on when MI_K2_STATE is unset)
    out += [make_case(m, None, False, "random") for m in ("ring65", "deg17_257", "deg33_130", "deg70_257")]
    # more than 1024 replicas: no threshold wavefront although none is turned off; 2 sweeps
    out += [make_case("ring130", state, False, "many", R=MANY_R, sweeps=2) for state in STATES]
    return out


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
assert len(BY_NAME) == len(CASES)
# one model of every width (and the padded, the partly flagged and the weighted one): its three state forms, with and
# without a threshold wavefront, must return the same run (tests/test_gpu_k2_state_forms.py)
SAME_RUN = ("ring65", "mixed257", "deg16_257", "deg17_257", "deg33_130", "deg70_257", "weighted137")


def forms_of(model_name):
    """The cases of one model from a random start, one per form K2 is built in for its width (the half form first)."""
    s = MODELS[model_name]
    scenario = "weighted" if s.heavy else "random"
    out = [make_case(model_name, None, False, scenario)]
    for state in ("byte", "bit"):
        out.append(make_case(model_name, state, False, scenario))
        if s.D in (16, 32):
            out.append(make_case(model_name, state, True, scenario))
    return out


# ---- the oracle ------------------------------------------------------------------------------------------------------------
def oracle(c, betas=None, R=None, init_dev=None, **kw):
    """oracle/sa_oracle.c on the device-side model of a case: states in DEVICE order [R, n_dev], energies, (proposals,
    accepted)."""
    d, m = device_model(c.model), model(c.model)
    run = dict(c.run)
    run.update(kw)
    st, en, stats = so.sa_csr_rank1_philox(d.rowptr, d.col, d.val, d.lin, m.c_pair, c.R if R is None else R,
                                           c.betas if betas is None else betas, c.seed, init=init_dev, weights=d.weights, **run)
    return st, en, (int(stats[0]), int(stats[1]))


def init_dev(c):
    if c.init is None:
        return None
    d = device_model(c.model)
    out = np.zeros((c.R, d.n_dev), dtype=np.uint8)
    out[:, d.seats] = c.init
    return out


@dataclasses.dataclass(frozen=True)
class Reference:
    states: np.ndarray           # device order; scenario "many": the picked slices, [len(MANY_PICKS) * MANY_WIDTH, n_dev]
    energies: np.ndarray
    proposals: int
    accepted: int


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle's run of a case, once per session and left unchanged."""
    c = BY_NAME[name] if isinstance(name, str) else name
    if c.scenario == "many":
        parts = [oracle(c, R=MANY_WIDTH, replica_offset=lo) for lo in MANY_PICKS]
        st, en = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        prop, acc = sum(p[2][0] for p in parts), sum(p[2][1] for p in parts)
    else:
        st, en, (prop, acc) = oracle(c, init_dev=init_dev(c))
    st.setflags(write=False)
    en.setflags(write=False)
    return Reference(st, en, prop, acc)


def replay(c):
    """The oracle's states after every sweep (device order, [sweeps + 1, R, n_dev], the first entry the initial states): the
    run continued sweep by sweep from the states and at the sweep offset it had reached."""
    R = MANY_WIDTH if c.scenario == "many" else c.R
    per_replica = c.scenario == "perbeta"
    base = c.run.get("sweep_offset", 0)
    start = oracle(c, betas=c.betas if per_replica else c.betas[:0], R=R, init_dev=init_dev(c),
                   **(dict(num_sweeps=0) if per_replica else {}))[0]
    out, acc = [start], 0
    for s in range(c.sweeps):
        kw = dict(num_sweeps=1) if per_replica else {}
        st, _, (_, a) = oracle(c, betas=c.betas if per_replica else c.betas[s:s + 1], R=R, init_dev=out[-1],
                               sweep_offset=base + s, **kw)
        out.append(st)
        acc += a
    return np.stack(out), acc
