"""Genes on which the negative-binomial fit (``mi_prep_nb_fit``) stalls, fails or sits on a decision edge, and which of them
the restatement (tests/sct_reference.py) itself answers firmly enough to hold the device to.  Numpy only, seeded; it loads no
library and never runs the device (tests/test_sct_edge_cases.py checks it, tests/test_gpu_sct_edges.py uses it).

Sizes are the kernel's edges: m = 3 (the entry's minimum: 253 lanes own no cell), 5, 64 (one wavefront), 256, 257 (one and two
cells per thread) and one block at 8192 cells (the LDS limit) with 8 genes.  Depths are 2000 exp(N(0, 0.5)).

The ensemble of a block is the restatement as it is, on four permutations of the cells, with the numpy port of the device's
psi functions, with every ``exp``, ``log`` and ``log1p`` one ulp up, then one ulp down, and eight times with the port, a
random last bit on every such result and a permutation together (another libm, another order; 3 + 1 at 8192 cells).  The
seven runs without the last eight pass genes that a further perturbation flips (a single count in the shallowest of 64 cells,
at the round limit in all seven and "converged" in round 31 under the next permutation), hence the eight.  ``s`` is a
gene's largest change over the ensemble: ``b0c`` and ``b1`` in their standard errors, alpha in ``se_alpha`` where that is
finite and positive and relative to alpha where not (a parameter without such a standard error is measured relative to
itself).  A gene QUALIFIES when ``poisson``, ``converged`` and the NaN / inf pattern of the six float outputs are the same in
every member, a gene that does not converge has 40 rounds in every member, and 100 s <= 1e-3 (the project's condition on TAU,
tests/test_gpu_sct.py, per gene).  The rest is ill-posed in the restatement itself: a flag or a NaN depends on the order of
summation, and no device can be held to that.  Most of the rest are the genes of ``runs_off``."""
import functools

import numpy as np

import sct_reference as sr

SIZES = (3, 5, 64, 256, 257, 8192)
FLOATS = ("b0c", "b1", "alpha", "se_b0c", "se_b1", "se_alpha")
PARAMETERS = (("b0c", "se_b0c"), ("b1", "se_b1"), ("alpha", "se_alpha"))
TWO24 = 16777216.0
CLASSES = {"a": "finite, not converged, l2 < 0 in the last round", "b": "failed: NaN b0 and b1",
           "c": "the 8 alpha bound in three successive rounds", "d": "the alpha / 8 bound or the quarter rule",
           "e": "Poisson by rule, b1 at rounding level", "f": "not Poisson, alpha < 1e-3", "g": "a count >= 2^24"}


SEEDS = {m: 7000 + m for m in SIZES}


def runs_off(Y, log_umi):
    """genes whose only non-zero count sits in the deepest or the shallowest cell.  Such a gene has no finite optimum: the
    slope runs off, the other cells' weights fall by a factor e per round, and with them both the stopping number, which
    passes 1e-16 after some 30 rounds, and the determinant of the 2 x 2 information matrix relative to its terms, which
    passes 2^-53 -- NaN -- in about the same round, 1e-16 being 2^-53.  Whether it ends "converged" on a meaningless iterate
    or failed is decided by rounding; the ensemble excludes nearly all of them at every size."""
    nz = Y != 0
    one = nz.sum(axis=0) == 1
    cell = nz.argmax(axis=0)
    return one & ((cell == np.argmax(log_umi)) | (cell == np.argmin(log_umi)))


def _families(rng, m, depth):
    """-> list of (family, counts (m,) float64, kept at the LDS limit)"""
    order = np.argsort(depth, kind="stable")                     # shallowest .. deepest
    ratio = depth / np.exp(np.log(depth).mean())
    deep = np.zeros(m, dtype=bool)
    out = []

    def add(family, y, at_limit=False):
        out.append((family, np.asarray(y, dtype=np.float64), at_limit))

    # the deepest and the shallowest cell, then interior ones (the median first)
    ranks = list(dict.fromkeys([m - 1, 0] + [int(round(f * (m - 1))) for f in (0.5, 0.2, 0.4, 0.6, 0.8)]))
    for count in (1.0, 7.0, 5000.0):
        for rank in ranks:
            y = np.zeros(m)
            y[order[rank]] = count
            add("single", y, count == 5000.0 and rank == ranks[2])
    for k, values in enumerate(([1, 2, 300, 4, 1], [3, 1, 1, 2000, 2], [40, 1, 1, 1, 1], [1, 1, 1, 1, 100000])):
        y = np.zeros(m)
        y[rng.permutation(m)[:min(len(values), m)]] = values[:min(len(values), m)]
        add("few_large", y, k == 0)
    for cut in (0.25, 0.5, 0.75):
        deep[:] = False
        deep[order[min(max(int(round(cut * m)), 1), m - 1):]] = True
        for height in (1.0, 4.0, 50.0):
            add("step", np.where(deep, height, 0.0), cut == 0.5 and height == 4.0)
            add("step", np.where(deep, 0.0, height))
    for c in (0.0, 1.0, 3.0, 1000.0):
        add("constant", np.full(m, c), c == 0.0)
    for mean in (0.3, 3.0, 30.0):
        for k in range(2):
            add("poisson", rng.poisson(mean * ratio), mean == 3.0 and k == 0)
        add("under_dispersed", np.round(mean * ratio), mean == 3.0)
    add("under_dispersed", np.round(300.0 * ratio))
    for theta in (1000.0, 100.0, 0.05, 0.01):
        for mean in (0.3, 3.0, 30.0):
            add("gamma_poisson", rng.poisson(rng.gamma(theta, mean * ratio / theta)), theta == 0.05 and mean == 3.0)
    for mean in (300.0, 1000.0):                                 # nearly Poisson, yet past the Poisson rule: alpha = 3.3e-4
        add("gamma_poisson", rng.poisson(rng.gamma(3000.0, mean * ratio / 3000.0)))
    add("large", rng.poisson(1e5 * ratio))
    for theta in (10.0, 3.0, 1.0, 0.3):
        add("large", rng.poisson(rng.gamma(theta, 1e5 * ratio / theta)))
    for rank in (m - 1, m // 2):
        y = rng.poisson(30.0 * ratio).astype(np.float64)
        y[order[rank]] = TWO24
        add("large", y, rank == m // 2)
    y = rng.poisson(1e5 * ratio).astype(np.float64)
    y[order[m // 2]] = 2.0 * TWO24
    add("large", y)
    for count in (1e5, 1e6, TWO24):                              # alone in the deepest cell: these run off, and fail before
        y = np.zeros(m)                                          # the stopping number is anywhere near 1e-16
        y[order[-1]] = count
        add("large", y)
    return out


@functools.lru_cache(maxsize=None)
def block(m, seed=None):
    """-> dict(Y (m x G, float32), log_umi (m,), family (G,) of names), read-only"""
    rng = np.random.default_rng(SEEDS[m] if seed is None else seed)
    depth = 2000.0 * np.exp(rng.normal(0.0, 0.5, m))
    genes = _families(rng, m, depth)
    if m == 8192:
        genes = [gene for gene in genes if gene[2]]
        assert len(genes) <= 8
    Y = np.column_stack([y for _, y, _ in genes]).astype(np.float32)
    out = dict(Y=np.ascontiguousarray(Y), log_umi=np.log10(depth), family=np.array([f for f, _, _ in genes]))
    for a in out.values():
        a.setflags(write=False)
    return out


def nudge_up(v):
    return np.nextafter(v, np.inf)


def nudge_down(v):
    return np.nextafter(v, -np.inf)


def random_nudge(seed):
    """every result one ulp up, one ulp down or as it is, drawn per element: another libm's last bit"""
    rng = np.random.default_rng(seed)

    def nudge(v):
        r = rng.integers(-1, 2, size=np.shape(v))
        return np.where(r > 0, np.nextafter(v, np.inf), np.where(r < 0, np.nextafter(v, -np.inf), v))
    return nudge


def members(Y, log_umi):
    """the ensemble: the base run (with its trace) first; then permutations of the cells, the ported psi pair, the two
    nudges, and runs with the ported pair and a random nudge on a permutation of their own.  (4 + 8 up to 1024 cells, 3 + 1
    above: a run at 8192 cells costs half a second.)"""
    n_perm, n_random = (4, 8) if len(log_umi) <= 1024 else (3, 1)
    perms = [np.random.default_rng(100 + k).permutation(len(log_umi)) for k in range(n_perm + n_random)]
    runs = [sr.nb_fit(Y, log_umi, trace=True)]
    runs += [sr.nb_fit(Y[p], log_umi[p]) for p in perms[:n_perm]]
    runs.append(sr.nb_fit(Y, log_umi, psi=sr.PORTED_PSI))
    runs += [sr.nb_fit(Y, log_umi, nudge=f) for f in (nudge_up, nudge_down)]
    runs += [sr.nb_fit(Y[p], log_umi[p], psi=sr.PORTED_PSI, nudge=random_nudge(200 + k)) for k, p in enumerate(perms[n_perm:])]
    return runs


def pattern(v):
    """0 finite, 1 NaN, 2 +inf, 3 -inf"""
    v = np.asarray(v, dtype=np.float64)
    return np.where(np.isnan(v), 1, np.where(v == np.inf, 2, np.where(v == -np.inf, 3, 0))).astype(np.int8)


def deviation(got, base, key, se_key):
    """|got - base[key]| per gene in the units of ``s``: base[se_key] where that is finite and positive, else |base[key]|;
    0 where the two are equal or both NaN, inf where they differ and there is no unit"""
    want, se = base[key], base[se_key]
    with np.errstate(all="ignore"):
        diff = np.abs(np.where((got == want) | (np.isnan(got) & np.isnan(want)), 0.0, got - want))
        unit = np.where(np.isfinite(se) & (se > 0), se, np.abs(want))
        return np.where(diff == 0, 0.0, np.where(unit > 0, diff / unit, np.inf))


def relative_spread(runs, key):
    """the largest relative change of a standard error over the ensemble (0 where all are equal or all NaN)"""
    base = runs[0][key]
    worst = np.zeros(len(base))
    with np.errstate(all="ignore"):
        for r in runs[1:]:
            same = (r[key] == base) | (np.isnan(r[key]) & np.isnan(base))
            worst = np.maximum(worst, np.where(same, 0.0, np.abs(r[key] - base) / np.abs(base)))
    return np.where(np.isnan(worst), np.inf, worst)


def qualify(runs):
    """-> dict(fit (the base run), s, qualifies, iterations_lo, iterations_hi, se_spread (3 x G)) of an ensemble"""
    base = runs[0]
    G = len(base["b1"])
    s = np.zeros(G)
    ok = np.ones(G, dtype=bool)
    for r in runs[1:]:
        ok &= (r["poisson"] == base["poisson"]) & (r["converged"] == base["converged"])
        for key in FLOATS:
            ok &= pattern(r[key]) == pattern(base[key])
        for key, se_key in PARAMETERS:
            s = np.maximum(s, deviation(r[key], base, key, se_key))
    its = np.array([r["iterations"] for r in runs])
    ok &= base["converged"] | (its == sr.MAX_ROUNDS).all(axis=0)
    ok &= 100.0 * s <= 1e-3
    return dict(fit=base, s=s, qualifies=ok, iterations_lo=its.min(axis=0), iterations_hi=its.max(axis=0),
                se_spread=np.array([relative_spread(runs, k) for k in ("se_b0c", "se_b1", "se_alpha")]))


def classes_of(Y, fit):
    """-> dict class letter -> bool per gene, from the base run and its trace"""
    tr = fit["trace"]
    G = Y.shape[1]
    last = np.maximum(fit["iterations"] - 1, 0)
    cols = np.arange(G)
    finite = np.isfinite(fit["b0c"]) & np.isfinite(fit["b1"]) & np.isfinite(fit["alpha"])
    high = tr["clamp"] == sr.CLAMP_HIGH
    low = (tr["clamp"] == sr.CLAMP_LOW) | (tr["rule"] == sr.RULE_QUARTER)
    with np.errstate(invalid="ignore"):
        flat = np.abs(fit["b1"]) <= 1e-9
        small = ~fit["poisson"] & (fit["alpha"] < 1e-3) & (fit["alpha"] > 0)
    return {"a": finite & ~fit["converged"] & ~fit["poisson"] & (tr["l2_sign"][last, cols] == -1),
            "b": np.isnan(fit["b0c"]) & np.isnan(fit["b1"]),
            "c": (high[:-2] & high[1:-1] & high[2:]).any(axis=0),
            "d": low.any(axis=0),
            "e": fit["poisson"] & fit["converged"] & flat,
            "f": small & fit["converged"],
            "g": (Y >= TWO24).any(axis=0)}


@functools.lru_cache(maxsize=None)
def qualified(m):
    """the block of size m with its ensemble's verdict and classes"""
    b = block(m)
    return qualified_block(b["Y"], b["log_umi"], block=b)


def qualified_block(Y, log_umi, **more):
    """qualify() of the ensemble of (Y, log_umi), with the classes and `own_lambda`: the largest stopping number over the
    members, each evaluated directly at its own final iterate (inf where one is NaN: the iterate sits where exp overflows)"""
    runs = members(Y, log_umi)
    q = qualify(runs)
    lam = np.array([sr.stop_number(Y, log_umi, r["b0c"], r["b1"], r["alpha"], r["poisson"]) for r in runs])
    q.update(classes=classes_of(Y, q["fit"]), own_lambda=np.where(np.isnan(lam).any(axis=0), np.inf, lam.max(axis=0)), **more)
    return q


def report():
    """-> (excluded share per (family, size), excluded share over all, qualifying genes per class), printed; the shares are
    over the genes that do not run off (runs_off), whose own count is printed"""
    shares, total, out, per_class = {}, 0, 0, dict.fromkeys(CLASSES, 0)
    for m in SIZES:
        q = qualified(m)
        fam = q["block"]["family"]
        off = runs_off(q["block"]["Y"], q["block"]["log_umi"])
        for f in np.unique(fam):
            shares[(f, m)] = float((~q["qualifies"][(fam == f) & ~off]).mean())
        total += int((~off).sum())
        out += int((~q["qualifies"] & ~off).sum())
        print("m = %4d: %d of the %d genes that run off are excluded" % (m, (~q["qualifies"] & off).sum(), off.sum()))
        for c in CLASSES:
            per_class[c] += int((q["classes"][c] & q["qualifies"]).sum())
        print("m = %4d: %3d genes, %d excluded, worst qualifying s %.3g, rounds %d .. %d" % (
            m, len(fam), (~q["qualifies"]).sum(), q["s"][q["qualifies"]].max(), q["fit"]["iterations"].min(),
            q["fit"]["iterations"].max()))
    print("excluded: %d of %d (%.1f %%); worst (family, size): %s" % (out, total, 100.0 * out / total,
                                                                      max(shares.items(), key=lambda kv: kv[1])))
    print("qualifying genes per class: " + ", ".join("(%s) %d" % kv for kv in per_class.items()))
    return shares, out / total, per_class
