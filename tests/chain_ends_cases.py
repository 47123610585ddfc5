"""The models of the chain-end tests (tests/test_chain_ends_host.py, tests/test_gpu_chain_ends.py): small structured models
in the caller's order and AS THE DEVICE HOLDS THEM (seat space for a padded layout), built the way engine.Problem builds
them.  TEST INFRASTRUCTURE ONLY."""
import dataclasses
import functools
from typing import Optional

import numpy as np

from scrna_seq_qannealing_clustering_amd import engine, models

VALUES = np.array([1 / 9, 0.25, 3 / 7, 2 / 3, 1.0, -0.5])
HEAVY_WEIGHTS = np.array([2, 4, 8, 16, 3, 5, 32])


def random_edges(rs, n, min_deg, max_deg):
    """A random graph with every degree in [min_deg, max_deg] (min_deg as far as the cap lets the last vertices reach it)."""
    deg = np.zeros(n, dtype=int)
    pairs = set()
    for i in range(n):
        tries = 0
        while deg[i] < max(min_deg, 1) and tries < 50 * max_deg:
            j = int(rs.randint(0, n))
            tries += 1
            if j == i or deg[j] >= max_deg or (min(i, j), max(i, j)) in pairs:
                continue
            pairs.add((min(i, j), max(i, j)))
            deg[i] += 1
            deg[j] += 1
    for _ in range(n * (max_deg - min_deg) // 4):                     # a spread of degrees above the floor
        i, j = (int(v) for v in rs.randint(0, n, 2))
        if i != j and deg[i] < max_deg and deg[j] < max_deg and (min(i, j), max(i, j)) not in pairs:
            pairs.add((min(i, j), max(i, j)))
            deg[i] += 1
            deg[j] += 1
    return sorted(pairs)


def hub_edges(rs, n, hub_deg):
    """A sparse ring and one hub of degree hub_deg: the runtime-width rows."""
    pairs = {(i, (i + 1) % n) if i + 1 < n else (0, i) for i in range(n)}
    for j in rs.choice(np.arange(1, n), size=hub_deg, replace=False):
        pairs.add((0, int(j)))
    pairs = {(min(a, b), max(a, b)) for a, b in pairs}
    while sum(1 for p in pairs if 0 in p) > hub_deg:
        pairs.discard(next(p for p in sorted(pairs, reverse=True) if 0 in p))
    return sorted(pairs)


@dataclasses.dataclass(frozen=True)
class Spec:
    n: int
    min_deg: int
    max_deg: int
    order: Optional[str]
    block: int
    c_pair: float
    heavy: int = 0               # binary: variables with pair-term weights behind the n coupled ones
    f64: bool = False            # binary: an fp64 energy model
    hub: bool = False


BINARY = {
    "b70": Spec(70, 0, 16, "padded", 64, 0.4),
    "b257": Spec(257, 17, 30, "padded", 64, -0.02),
    "b128": Spec(257, 0, 9, "padded", 128, 0.4),
    "b256": Spec(257, 0, 9, "padded", 256, -0.02),
    "hub70": Spec(257, 0, 70, None, 64, 0.0, hub=True),
    "wgt": Spec(130, 0, 9, "padded", 64, 0.4, heavy=7),
    "f64": Spec(70, 0, 16, "padded", 64, -0.02, f64=True),
    "c0": Spec(70, 0, 16, "padded", 64, 0.0),
}
POTTS = {
    "p70": Spec(70, 0, 9, "padded", 64, 0.4),
    "p257": Spec(257, 0, 16, "padded", 64, -0.02),
    "p257w": Spec(257, 17, 30, "padded", 64, 0.4),
    "phub": Spec(257, 0, 70, None, 64, -0.02, hub=True),
}


@dataclasses.dataclass(frozen=True)
class Model:
    """Caller's order (fp32 chain coefficients, fp64 ones of the energy model) and device order."""
    spec: Spec
    n: int
    rowptr: np.ndarray
    col: np.ndarray
    val: np.ndarray
    lin: np.ndarray
    val64: np.ndarray
    lin64: np.ndarray
    c_pair: float
    c64: float
    weights: Optional[np.ndarray]
    n_dev: int
    seats: np.ndarray
    d_rowptr: np.ndarray
    d_col: np.ndarray
    d_val: np.ndarray
    d_lin: np.ndarray
    d_val64: np.ndarray
    d_lin64: np.ndarray
    d_weights: Optional[np.ndarray]

    def to_device(self, X, dtype):
        out = np.zeros((len(X), self.n_dev), dtype=dtype)
        out[:, self.seats] = X
        return out

    @property
    def present(self):
        out = np.zeros(self.n_dev, dtype=bool)
        out[self.seats] = True
        return out


def _edges(s, rs):
    return hub_edges(rs, s.n, s.max_deg) if s.hub else random_edges(rs, s.n, s.min_deg, s.max_deg)


@functools.lru_cache(maxsize=None)
def model(name):
    s = (BINARY.get(name) or POTTS[name])
    rs = np.random.RandomState(9000 + sorted(list(BINARY) + list(POTTS)).index(name))
    e = np.asarray(_edges(s, rs), dtype=np.int64).reshape(-1, 2)
    rowptr, col, val64 = models._csr_from_edges(s.n, e[:, 0], e[:, 1], rs.choice(VALUES, size=len(e)))
    rowptr, col = rowptr.astype(np.int32), col.astype(np.int32)
    lin64 = rs.normal(scale=0.7, size=s.n)
    n, weights = s.n, None
    if s.heavy:
        n = s.n + s.heavy
        rowptr = np.concatenate([rowptr, [rowptr[-1]] * s.heavy]).astype(np.int32)
        lin64 = np.concatenate([lin64, rs.normal(scale=0.3, size=s.heavy)])
        weights = np.concatenate([np.ones(s.n, dtype=np.int64), HEAVY_WEIGHTS[:s.heavy]])
    val, lin = val64.astype(np.float32), lin64.astype(np.float32)
    c32 = float(np.float32(s.c_pair))
    d_w = None
    if weights is not None:
        rp, cc, vv, dl, d_w, seats, n_dev, dv64, dl64 = engine.weighted_layout_csr(
            rowptr, col, val, lin, weights, energy_model=(val64, lin64, s.c_pair))
    elif s.order == "padded":
        seats, nslots, clashes = models.padded_slot_layout(rowptr, col, slot=s.block)
        assert clashes == 0
        if s.block == 128 and nslots % 2:
            nslots += 1
        n_dev = nslots * s.block
        rp, cc, vv, dv64 = models.pad_csr(rowptr, col, val, seats, n_dev, also=val64)
        dl = np.full(n_dev, np.inf, dtype=np.float32)
        dl[seats] = lin
        dl64 = np.zeros(n_dev)
        dl64[seats] = lin64
    else:
        rp, cc, vv, dv64, dl, dl64, seats, n_dev = rowptr, col, val, val64, lin, lin64, np.arange(n), n
    out = Model(s, n, rowptr, col, val, lin, val64, lin64, c32, float(s.c_pair), weights, int(n_dev),
                np.asarray(seats, dtype=np.int64), np.asarray(rp, dtype=np.int32), np.asarray(cc, dtype=np.int32),
                np.asarray(vv, dtype=np.float32), np.asarray(dl, dtype=np.float32), np.asarray(dv64, dtype=np.float64),
                np.asarray(dl64, dtype=np.float64), d_w)
    for f in dataclasses.fields(out):
        if isinstance(getattr(out, f.name), np.ndarray):
            getattr(out, f.name).setflags(write=False)
    return out


def binary_reference_args(m):
    """What chain_ends_reference.binary_energy takes after the states: the coefficients the device sums."""
    if m.spec.f64:
        return (m.d_rowptr, m.d_col, m.d_val64, m.d_lin64, m.c64)
    return (m.d_rowptr, m.d_col, m.d_val, m.d_lin, m.c_pair)


def node_weights(m, groups=2):
    """Integer node weights, their fp32 move coefficients and fp64 energy weights (caller's order), and per resolution
    group: coefficients [G, n], fp64 pair coefficient and energy offset."""
    rs = np.random.RandomState(77 + m.n)
    wq = rs.randint(1, 9, size=m.n).astype(np.int32)
    w64 = wq * 0.37
    c64 = np.array([0.013 * (g + 1) for g in range(groups)])
    cw = np.stack([(c64[g] * 0.37 * 0.37 * wq).astype(np.float32) for g in range(groups)])
    offset = np.array([-1.5 * (g + 1) for g in range(groups)])
    return wq, cw, w64, c64, offset
