"""Independent reference for the statistical tests of the annealing chains.  Plain numpy, fp64.

Everything here is written from the model definitions of DESIGN.md section 3 alone: it imports neither ``oracle/`` nor
the package, so a test built on it can disagree with both.  A sequential Metropolis sweep leaves ``exp(-beta E)``
invariant, so at a constant beta, after burn-in, the replicas of a run are independent samples of the Boltzmann
distribution of a model small enough to enumerate:

* ``enumerate_binary`` / ``enumerate_potts``: every state and its fp64 energy (fp32 coefficients widened first);
* ``boltzmann``: the normalised distribution, optionally restricted to an allowed set of states;
* ``reference``: that distribution after the condition on the model (pooled mass), settled before a chain runs;
* ``chi_square``: Pearson's statistic of observed state counts, the bins that expect fewer than 5 pooled into one;
* ``energy_z``: z-score of the mean reported energy, after checking every reported energy against its state's;
* ``accept_moments_*``: exact mean and variance of the number of accepted moves of ONE replica over sweeps that start
  from a given distribution (the stationary one in the tests), by propagating the zeroth, first and second moment of
  the running count through every proposal of the sweep.  The propagated distribution is returned too: it must still
  be the Boltzmann one, which checks the reference against itself.

PASS RULE (fixed; seeds are fixed and the chains are bit-reproducible, so every case is deterministic):
p >= 1e-6, |z| <= 5, at most one pooled bin holding at most 5 % of the probability mass, and -- where a case counts
accepted moves -- the count within 5 standard errors of its expectation.
"""
import numpy as np
from scipy import stats as _st

P_MIN = 1e-6            # chi-square p-value a stationary chain must reach
Z_MAX = 5.0             # |z| of the mean energy / of the accepted-move count
POOL_MAX = 0.05         # probability mass the pooled bin may hold
P_REJECT = 1e-12        # what a chain that does NOT sample the distribution must stay below (power checks)


# ---------------------------------------------------------------------------------------------------------------------
# states
def binary_states(n):
    """[2^n, n] uint8; state number ``sum_i x_i << i``."""
    return ((np.arange(1 << n, dtype=np.int64)[:, None] >> np.arange(n)) & 1).astype(np.uint8)


def binary_index(states):
    states = np.asarray(states)
    return (states.astype(np.int64) << np.arange(states.shape[1], dtype=np.int64)).sum(axis=1)


def potts_states(n, K):
    """[K^n, n] int64; state number ``sum_i l_i K^i``."""
    return (np.arange(K ** n, dtype=np.int64)[:, None] // (K ** np.arange(n, dtype=np.int64))) % K


def potts_index(labels, K):
    labels = np.asarray(labels)
    return (labels.astype(np.int64) * (K ** np.arange(labels.shape[1], dtype=np.int64))).sum(axis=1)


def _upper_edges(rowptr, col, val):
    """(u, v, S_uv as fp64) of the stored entries with u < v of a symmetric CSR matrix (every edge once)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    row = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    col = np.asarray(col, dtype=np.int64)
    val = np.asarray(val, dtype=np.float32).astype(np.float64)
    keep = col > row
    return row[keep], col[keep], val[keep]


# ---------------------------------------------------------------------------------------------------------------------
# energies
def enumerate_binary(Qs=None, rowptr=None, col=None, val=None, lin=None, c_pair=0.0, weights=None):
    """All 2^n states and their fp64 energies.

    Dense (``Qs`` symmetric fp32, diagonal = linear terms): ``sum_i Qs_ii x_i + 2 sum_{i<j} Qs_ij x_i x_j``.
    Structured (symmetric CSR ``S``, ``lin``, ``c_pair``): ``sum_i lin_i x_i + sum_{i<j} S_ij x_i x_j + c s (s - 1) / 2``,
    ``s = sum x``; with integer ``weights`` a the pair term is ``c a_i a_j`` on every pair,
    ``c / 2 ((sum a_i x_i)^2 - sum a_i^2 x_i)``."""
    if Qs is not None:
        Q = np.asarray(Qs, dtype=np.float32).astype(np.float64)
        n = Q.shape[0]
        X = binary_states(n)
        Xd = X.astype(np.float64)
        E = Xd @ np.diag(Q).copy() + np.einsum("si,ij,sj->s", Xd, 2.0 * np.triu(Q, 1), Xd)
        return X, E
    lin = np.asarray(lin, dtype=np.float32).astype(np.float64)
    n = len(lin)
    X = binary_states(n)
    Xd = X.astype(np.float64)
    E = Xd @ lin
    for u, v, s in zip(*_upper_edges(rowptr, col, val)):
        E += s * Xd[:, u] * Xd[:, v]
    c = np.float64(np.float32(c_pair))
    a = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    A = Xd @ a
    E += c * 0.5 * (A * A - Xd @ (a * a))
    return X, E


def enumerate_potts(rowptr, col, val, c_pair, n, K, node_weights=None):
    """All K^n labelings and their fp64 energies: ``sum_{u<v, same label} S_uv + c sum_q C(N_q, 2)``; with node weights
    w the size term is ``c sum_q (W_q^2 - sum_{i in q} w_i^2) / 2``, ``W_q`` the weight of cluster q."""
    L = potts_states(n, K)
    E = np.zeros(len(L))
    for u, v, s in zip(*_upper_edges(rowptr, col, val)):
        E += s * (L[:, u] == L[:, v])
    c = np.float64(np.float32(c_pair)) if node_weights is None else np.float64(c_pair)
    w = np.ones(n) if node_weights is None else np.asarray(node_weights, dtype=np.float64)
    for q in range(K):
        m = (L == q).astype(np.float64)
        W = m @ w
        E += c * 0.5 * (W * W - m @ (w * w))
    return L, E


def potts_allowed(L, K, min_size):
    """Labelings in which every cluster holds at least ``min_size`` variables."""
    ok = np.ones(len(L), dtype=bool)
    for q in range(K):
        ok &= (L == q).sum(axis=1) >= min_size
    return ok


# ---------------------------------------------------------------------------------------------------------------------
# statistics
def boltzmann(E, beta, allowed=None):
    E = np.asarray(E, dtype=np.float64)
    w = np.exp(-np.float64(beta) * (E - E.min()))
    if allowed is not None:
        w = np.where(allowed, w, 0.0)
    return w / w.sum()


def chi_square(counts, p):
    """Pearson chi-square of ``counts`` against the distribution ``p``; the bins that expect fewer than 5 are pooled into
    one.  Returns ``(chi2, degrees of freedom, p-value, pooled probability mass, pooled bins)``.  Bins of probability
    zero (states outside a restricted set) belong to the pooled bin: a single sample there costs ``1 / expectation``."""
    counts = np.asarray(counts, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    expect = p * counts.sum()
    small = expect < 5.0
    obs, exp = counts[~small], expect[~small]
    if small.any():
        po, pe = counts[small].sum(), expect[small].sum()
        if pe > 0.0:
            obs, exp = np.append(obs, po), np.append(exp, pe)
        elif po > 0.0:
            return np.inf, max(len(exp) - 1, 1), 0.0, 0.0, int(small.sum())
    x2 = float(((obs - exp) ** 2 / exp).sum())
    df = max(len(exp) - 1, 1)
    return x2, df, float(_st.chi2.sf(x2, df)), float(p[small].sum()), int(small.sum())


def energy_z(energies, index, E, p, atol):
    """z-score of the mean reported energy against the enumerated mean; every reported energy must equal the
    enumerated energy of the state reported with it (``index``) to ``atol``."""
    energies = np.asarray(energies, dtype=np.float64)
    worst = float(np.abs(energies - E[index]).max())
    assert worst <= atol, "a reported energy is %.3g away from its state's enumerated energy" % worst
    mu = float((p * E).sum())
    var = float((p * (E - mu) ** 2).sum())
    if var == 0.0:
        return 0.0
    return float((energies.mean() - mu) / np.sqrt(var / len(energies)))


def _moments_step(m, src, dst, a):
    """One proposal on the moment vectors m = (m0, m1, m2): the states ``src`` move to ``dst`` with probability ``a``
    (and count one accepted move), else stay."""
    m0, m1, m2 = m
    o0, o1, o2 = m0.copy(), m1.copy(), m2.copy()
    f0, f1, f2 = m0[src] * a, m1[src] * a, m2[src] * a
    np.subtract.at(o0, src, f0)
    np.subtract.at(o1, src, f1)
    np.subtract.at(o2, src, f2)
    np.add.at(o0, dst, f0)
    np.add.at(o1, dst, f1 + f0)
    np.add.at(o2, dst, f2 + 2.0 * f1 + f0)
    return o0, o1, o2


def accept_moments_binary(E, n, beta, p0, sweeps=1, sites=None):
    """Exact ``(mean, variance, final distribution)`` of one replica's accepted-move count over ``sweeps`` sequential
    sweeps of single-bit Metropolis proposals (``sites``: the variables proposed, default all, in index order) started
    from the distribution ``p0``."""
    E = np.asarray(E, dtype=np.float64)
    idx = np.arange(len(E))
    m = (np.asarray(p0, dtype=np.float64).copy(), np.zeros(len(E)), np.zeros(len(E)))
    for _ in range(sweeps):
        for i in (range(n) if sites is None else sites):
            dst = idx ^ (1 << i)
            a = np.minimum(1.0, np.exp(-beta * (E[dst] - E)))
            m = _moments_step(m, idx, dst, a)
    mean = m[1].sum()
    return float(mean), float(m[2].sum() - mean * mean), m[0]


def accept_moments_potts(E, n, K, beta, p0, sweeps=1, min_size=0, sites=None):
    """The same for the Potts chain: variable i with label a proposes each of the K - 1 other labels with equal
    probability; a move that would leave fewer than ``min_size`` variables in a is rejected."""
    E = np.asarray(E, dtype=np.float64)
    L = potts_states(n, K)
    idx = np.arange(len(E))
    sizes = np.stack([(L == q).sum(axis=1) for q in range(K)], axis=1)
    m = (np.asarray(p0, dtype=np.float64).copy(), np.zeros(len(E)), np.zeros(len(E)))
    for _ in range(sweeps):
        for i in (range(n) if sites is None else sites):
            a_lab = L[:, i]
            own = sizes[idx, a_lab]
            # the K - 1 targets are exclusive outcomes of ONE proposal: all flows leave the pre-proposal moments
            flows = []
            for d in range(1, K):
                b_lab = (a_lab + d) % K
                dst = idx + (b_lab - a_lab) * K ** i
                a = np.minimum(1.0, np.exp(-beta * (E[dst] - E))) / (K - 1)
                a = np.where(own - 1 >= min_size, a, 0.0)
                flows.append((dst, m[0] * a, m[1] * a, m[2] * a))
            o0, o1, o2 = m[0].copy(), m[1].copy(), m[2].copy()
            for dst, f0, f1, f2 in flows:
                o0 -= f0
                o1 -= f1
                o2 -= f2
                np.add.at(o0, dst, f0)
                np.add.at(o1, dst, f1 + f0)
                np.add.at(o2, dst, f2 + 2.0 * f1 + f0)
            m = (o0, o1, o2)
    mean = m[1].sum()
    return float(mean), float(m[2].sum() - mean * mean), m[0]


def accept_z(accepted, replicas, mean, var):
    """z-score of a run's total accepted-move count: ``replicas`` independent replicas, each with the given moments."""
    if var <= 0.0:
        assert accepted == round(replicas * mean), (accepted, replicas * mean)
        return 0.0
    return float((accepted - replicas * mean) / np.sqrt(replicas * var))


# ---------------------------------------------------------------------------------------------------------------------
# the pass rule
def reference(E, beta, samples, allowed=None):
    """The Boltzmann distribution a case is judged against, after the condition on the MODEL -- settled from the
    enumeration alone, BEFORE the chain runs: the bins that expect fewer than 5 of ``samples`` hold at most 5 % of the
    mass."""
    p = boltzmann(E, beta, allowed)
    pooled = float(p[p * samples < 5.0].sum())
    assert pooled <= POOL_MAX, "the pooled bin would hold %.3f of the mass: choose another model or beta" % pooled
    return p


def judge(name, index, energies, E, p, atol, accepted=None, acc_moments=None):
    """Apply the pass rule to one run: ``index`` the state number of every replica, ``energies`` what the engine reported
    for it; ``accepted`` / ``acc_moments`` = (mean, var) per replica for the accepted-move check.  Prints the figures,
    then asserts."""
    x2, df, pv, pooled, bins = chi_square(np.bincount(index, minlength=len(E)), p)
    z = energy_z(energies, index, E, p, atol)
    acc_z = None if accepted is None else accept_z(accepted, len(index), acc_moments[0], acc_moments[1])
    print("%-44s chi2 %9.1f / %4d  p %.3g  z %+.2f  pooled %.4f (%d bins)%s" % (
        name, x2, df, pv, z, pooled, bins, "" if acc_z is None else "  acc %+.2f s.e." % acc_z))
    assert pooled <= POOL_MAX, "the pooled bin holds %.3f of the mass: choose another model or beta" % pooled
    assert pv >= P_MIN, "%s: chi-square rejects the Boltzmann distribution (p = %.3g)" % (name, pv)
    assert abs(z) <= Z_MAX, "%s: mean energy %.2f standard errors off" % (name, z)
    if acc_z is not None:
        assert abs(acc_z) <= Z_MAX, "%s: accepted-move count %.2f standard errors off" % (name, acc_z)


# ---------------------------------------------------------------------------------------------------------------------
# the small models of the tests (shared by the CPU and the GPU file so both judge the same distributions)
def random_dense(n, seed):
    """Symmetric fp32 matrix of standard normal entries (diagonal = linear terms)."""
    A = np.random.RandomState(seed).randn(n, n)
    return np.ascontiguousarray(((A + A.T) / 2).astype(np.float32))


def random_graph(n, seed, density=0.4):
    """Symmetric CSR ``(rowptr, col, val)`` of a random graph with NEGATIVE couplings in (-1, 0), rows sorted by column;
    a spanning path keeps it connected."""
    rng = np.random.RandomState(seed)
    iu, ju = np.triu_indices(n, 1)
    keep = (rng.rand(len(iu)) < density) | (ju == iu + 1)
    w = (-rng.rand(len(iu))).astype(np.float32)
    S = np.zeros((n, n), dtype=np.float32)
    S[iu[keep], ju[keep]] = w[keep]
    S = S + S.T
    rowptr, col, val = [0], [], []
    for i in range(n):
        nz = np.flatnonzero(S[i])
        col.extend(nz.tolist())
        val.extend(S[i, nz].tolist())
        rowptr.append(len(col))
    return np.asarray(rowptr, dtype=np.int32), np.asarray(col, dtype=np.int32), np.asarray(val, dtype=np.float32)


def embed_dense(Qs, n_total, diag=64.0):
    """``Qs`` as the leading block of an ``n_total`` matrix whose other variables are uncoupled with linear term
    ``diag``: with beta * diag above 16 (the largest -ln u the chains draw is 23 ln 2 = 15.9) such a variable, once 0,
    never flips again, and it leaves 1 at its first proposal."""
    n = Qs.shape[0]
    out = np.zeros((n_total, n_total), dtype=np.float32)
    out[:n, :n] = Qs
    out[np.arange(n, n_total), np.arange(n, n_total)] = np.float32(diag)
    return out


def csr_model(kind):
    """n = 9: a random sparse graph with negative couplings, random linear terms, and a pair term -- none (``c0``),
    uniform (``pair``), or weighted with two slack-like variables of weight 2 and 4 that have no couplings."""
    lin = (np.random.RandomState(22).randn(9) * 0.5).astype(np.float32)
    if kind == "weighted":
        rp, col, val = random_graph(7, 23)
        rp = np.concatenate([rp, [rp[-1]] * 2]).astype(np.int32)
        lin[7:] = (0.3, -0.2)
        return rp, col, val, lin, 0.11, np.array([1] * 7 + [2, 4])
    rp, col, val = random_graph(9, 21)
    return rp, col, val, lin, (0.0 if kind == "c0" else 0.11), None


def potts_model(n, scale=1.0):
    """A random graph on n variables with couplings in (-scale, 0) and pair coefficient 0.2 scale."""
    rp, col, val = random_graph(n, 30 + n)
    return rp, col, (val * np.float32(scale)).astype(np.float32), 0.2 * scale


HUB_BLOCK, HUB_FREE = 12, 5


def hub_model():
    """n = 18, K = 2, for the Potts kernels built for rows of 17 .. 32 stored entries: variable 0 is coupled to all 17
    others.  2^18 labelings cannot each expect 5 of 2^18 samples, so 12 of the leaves are tied to the hub with a coupling
    of -20: a labeling with one of them off the hub's label has weight e^-20 beta and falls into the pooled bin, and the
    hub and its 12 move as ONE variable -- which single-site moves never relabel after the first sweep.  Which label the
    block takes is settled by symmetry, not by mixing: with K = 2 the energy, the proposal rule and the tag-1 initial law
    are all invariant under swapping the labels, so the block holds either label with probability exactly 1/2, as in
    the Boltzmann distribution.  The other 5 leaves (couplings in (-1, 0) to the hub, a path among themselves) mix
    freely: 2 x 32 labelings carry the mass.  Returns (rowptr, col, val, c_pair)."""
    n = 1 + HUB_BLOCK + HUB_FREE
    rng = np.random.RandomState(41)
    S = np.zeros((n, n), dtype=np.float32)
    S[0, 1:1 + HUB_BLOCK] = -20.0
    S[0, 1 + HUB_BLOCK:] = (-rng.rand(HUB_FREE)).astype(np.float32)
    for i in range(1 + HUB_BLOCK, n - 1):
        S[i, i + 1] = np.float32(-rng.rand())
    S = S + S.T
    rowptr, col, val = [0], [], []
    for i in range(n):
        nz = np.flatnonzero(S[i])
        col.extend(nz.tolist())
        val.extend(S[i, nz].tolist())
        rowptr.append(len(col))
    return np.asarray(rowptr, dtype=np.int32), np.asarray(col, dtype=np.int32), np.asarray(val, dtype=np.float32), 0.05


PT_LADDER = np.array([0.3, 0.6, 1.2, 2.4])
PT_CHAINS = 1 << 16


def judge_rungs(name, states, energies, rung, E, atol, accepted=None):
    """Parallel tempering: the replicas that hold rung k against the Boltzmann distribution at beta_k, per rung; with
    ``accepted`` -- the moves ONE further sweep at the rungs' temperatures accepted, over all replicas -- that count
    against the sum of the rungs' exact moments (2^16 independent replicas per rung)."""
    mean = var = 0.0
    for k, beta in enumerate(PT_LADDER):
        on = rung == k
        assert on.sum() == PT_CHAINS
        p = boltzmann(E, beta)
        judge("%s rung %d beta=%g" % (name, k, beta), binary_index(states[on]), energies[on], E, p, atol)
        m = accept_moments_binary(E, states.shape[1], beta, p)
        mean, var = mean + PT_CHAINS * m[0], var + PT_CHAINS * m[1]
    if accepted is not None:
        z = float((accepted - mean) / np.sqrt(var))
        print("%-44s accepted moves of one further sweep, all rungs: %+.2f s.e." % (name, z))
        assert abs(z) <= Z_MAX, "%s: accepted-move count %.2f standard errors off" % (name, z)
