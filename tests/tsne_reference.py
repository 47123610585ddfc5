"""Chain T restated in numpy: every stage in fp64, and a float32 evaluation of the layout whose
distance to the fp64 one is D32.  TEST INFRASTRUCTURE ONLY: dense n x n arrays, small n."""
import numpy as np

CALIBRATION_STEPS = 100


# ---- T1 ------------------------------------------------------------------------------------------------------------------------

def knn_lexsort(X, K):
    """(nn, d2): the K nearest OTHER points by ascending (d2, index), d2 exact in fp64 from the f32 coordinates and rounded to
    f32 (on small-integer lattices that is the f32 fmaf chain's value, exactly)."""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    n = len(X64)
    D = np.zeros((n, n))
    for c in range(X64.shape[1]):
        D += (X64[:, None, c] - X64[None, :, c]) ** 2
    nn = np.empty((n, K), dtype=np.int32)
    for i in range(n):
        idx = np.delete(np.arange(n), i)
        order = np.lexsort((idx, D[i, idx]))[:K]
        nn[i] = idx[order]
    return nn, np.take_along_axis(D, nn.astype(np.int64), axis=1).astype(np.float32)


# ---- T2 ------------------------------------------------------------------------------------------------------------------------

def entropy(D, beta):
    """(H, p, Z) of rows D (already shifted by their minimum) at beta; sums in column order"""
    p = np.exp(-(beta[:, None] * D))
    Z = np.zeros(len(D))
    S = np.zeros(len(D))
    for j in range(D.shape[1]):
        Z = Z + p[:, j]
        S = S + p[:, j] * D[:, j]
    return np.log(Z) + beta * S / Z, p, Z


def calibrate(d2, perplexity, steps=CALIBRATION_STEPS):
    """(beta, cond, H): van der Maaten's bisection, exactly `steps` steps from beta = 1 with bounds -inf, +inf, no tolerance
    exit; cond = the conditional rows at the final beta, H their entropy (nats)."""
    d2 = np.asarray(d2, dtype=np.float32).astype(np.float64)
    D = d2 - d2[:, :1]
    n = len(D)
    target = np.log(float(perplexity))
    beta, lo, hi = np.ones(n), np.full(n, -np.inf), np.full(n, np.inf)
    with np.errstate(over="ignore", invalid="ignore"):
        for _ in range(steps):
            H = entropy(D, beta)[0]
            up = H > target
            lo = np.where(up, beta, lo)
            hi = np.where(up, hi, beta)
            beta = np.where(up, np.where(np.isinf(hi), beta * 2.0, (beta + hi) / 2.0),
                            np.where(np.isinf(lo), beta / 2.0, (beta + lo) / 2.0))
    H, p, Z = entropy(D, beta)
    return beta, p / Z[:, None], H


# ---- T3 ------------------------------------------------------------------------------------------------------------------------

def joint(nn, cond):
    """(rowptr, col, P64, P32): P_ij = (p_j|i + p_i|j) / (2 n) over the union of the pattern, fp64, stored as f32; entries
    whose stored value is 0 are dropped"""
    n, K = nn.shape
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), K), nn.ravel()] = np.asarray(cond, dtype=np.float64).ravel()
    P = (A + A.T) / (2.0 * n)
    P32 = P.astype(np.float32)
    keep = P32 > 0
    rows, col = np.nonzero(keep)
    rowptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    return rowptr, col.astype(np.int32), P[rows, col], P32[rows, col]


def affinities(X, perplexity):
    K = int(np.floor(3.0 * perplexity))
    nn, d2 = knn_lexsort(X, K)
    beta, cond, _ = calibrate(d2, perplexity)
    rowptr, col, _, P32 = joint(nn, cond)
    return nn, d2, beta, cond, rowptr, col, P32


# ---- T4 ------------------------------------------------------------------------------------------------------------------------

def dense(rowptr, col, P, dtype=np.float64):
    n = len(rowptr) - 1
    M = np.zeros((n, n), dtype=dtype)
    M[np.repeat(np.arange(n), np.diff(rowptr)), col] = np.asarray(P, dtype=np.float32).astype(dtype)
    return M


def gradient(Pd, Y, exag, dtype=np.float64, mutate=None):
    """(g, Z): g_i = exag sum_j P_ij q_ij (y_i - y_j) - (sum_{j != i} q_ij^2 (y_i - y_j)) / Z, every pair term in `dtype`,
    Z in fp64 (rounded to `dtype` for the division, as the kernel rounds it to f32)."""
    Y = np.asarray(Y, dtype=dtype)
    n = len(Y)
    diff = Y[:, None, :] - Y[None, :, :]
    s = (diff * diff).sum(axis=2, dtype=dtype)
    q = (dtype(1.0) / (dtype(1.0) + s)).astype(dtype)
    q[np.arange(n), np.arange(n)] = 0
    Z = float(q.sum(dtype=np.float64))
    if mutate == "z_half":
        Z = float(np.triu(q, 1).sum(dtype=np.float64))
    attr = ((Pd * q)[:, :, None] * diff).sum(axis=1, dtype=dtype)
    rep = ((q * q)[:, :, None] * diff).sum(axis=1, dtype=dtype)
    g = dtype(exag) * attr - rep / dtype(Z)
    if mutate == "factor4":
        g = dtype(4.0) * g
    return g.astype(dtype), Z


def layout(rowptr, col, P, Y0, eta, exag, exag_iters, m0, m1, switch_iter, T, t0=0, U0=None, gains0=None, center=True,
           dtype=np.float64, mutate=None):
    """-> (Y, U, gains, Z of the last iteration): bhtsne's iteration t = t0 .. t0 + T - 1 with the exact repulsion, in `dtype`;
    the column means (fp64, rounded to f32) leave once, after the last iteration.  mutate: one of the mistakes
    tests/test_tsne_host.py must be able to see ("exag_switch", "mom_switch", "z_half", "gain_inverted", "factor4")."""
    Pd = dense(rowptr, col, P, dtype)
    Y = np.asarray(Y0, dtype=np.float32).astype(dtype)
    U = np.zeros_like(Y) if U0 is None else np.asarray(U0, dtype=np.float32).astype(dtype)
    gains = np.ones_like(Y) if gains0 is None else np.asarray(gains0, dtype=np.float32).astype(dtype)
    eta, m0, m1 = (dtype(np.float32(v)) for v in (eta, m0, m1))
    exag = dtype(np.float32(exag))
    Z = 0.0
    for t in range(t0, t0 + T):
        e_t = exag if t < exag_iters + (1 if mutate == "exag_switch" else 0) else dtype(1.0)
        m_t = m0 if t < switch_iter + (1 if mutate == "mom_switch" else 0) else m1
        g, Z = gradient(Pd, Y, e_t, dtype, mutate)
        differ = np.sign(g) != np.sign(U)
        if mutate == "gain_inverted":
            differ = ~differ
        gains = np.where(differ, gains + dtype(0.2), gains * dtype(0.8)).astype(dtype)
        gains = np.maximum(gains, dtype(0.01))
        U = (m_t * U - (eta * gains) * g).astype(dtype)
        Y = (Y + U).astype(dtype)
    if center:
        mean = Y.astype(np.float64).mean(axis=0) if dtype is np.float64 else \
            np.float32(Y.astype(np.float32).astype(np.float64).mean(axis=0))
        Y = (Y - mean.astype(dtype)).astype(dtype)
    return Y, U, gains, Z


def kl(rowptr, col, P, Y):
    """sum over the stored entries of P log(P Z / q) in fp64, from the coordinates as given"""
    Y = np.asarray(Y, dtype=np.float64)
    n = len(Y)
    s = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2)
    q = 1.0 / (1.0 + s)
    q[np.arange(n), np.arange(n)] = 0.0
    Z = q.sum()
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    p = np.asarray(P, dtype=np.float32).astype(np.float64)
    return float((p * np.log(p * Z / q[rows, col])).sum())


# ---- inputs --------------------------------------------------------------------------------------------------------------------

def blobs(seed=0, n=300, dim=10, sep=50.0):
    """three unit-variance Gaussian blobs whose centres are `sep` standard deviations apart (an equilateral triangle)"""
    rng = np.random.default_rng(seed)
    centres = np.zeros((3, dim))
    centres[1, 0] = sep
    centres[2, 0], centres[2, 1] = sep / 2.0, sep * np.sqrt(3.0) / 2.0
    labels = np.arange(n) % 3
    return (centres[labels] + rng.normal(size=(n, dim))).astype(np.float32), labels


def lattice(n, dim, side, seed):
    """n points with small-integer coordinates in [0, side): every f32 squared distance is exact and ties abound"""
    return np.random.default_rng(seed).integers(0, side, size=(n, dim)).astype(np.float32)


def sparse_graph(n, per_row, empty=(), hub=None, hub_deg=0, seed=0):
    """A symmetric CSR whose weights sum to 1 (a joint distribution): a ring over the rows not in `empty`, vertex `hub` joined
    to hub_deg vertices in all, random pairs up to about `per_row` entries per row; weights U(0.15, 1) / their sum."""
    rng = np.random.default_rng(seed)
    live = np.array([v for v in range(n) if v not in set(empty)])
    W = np.zeros((n, n))
    if len(live) > 2:
        W[live, np.roll(live, -1)] = rng.uniform(0.15, 1.0, size=len(live))
    elif len(live) == 2:
        W[live[0], live[1]] = rng.uniform(0.15, 1.0)
    if per_row > 2:
        mask = np.zeros((n, n), dtype=bool)
        mask[np.ix_(live, live)] = rng.random((len(live), len(live))) < (per_row - 2.0) / (2.0 * max(len(live) - 1, 1))
        W = np.where((W == 0) & mask, rng.uniform(0.15, 1.0, size=(n, n)), W)
    if hub is not None:
        others = np.array([v for v in live if v != hub])
        pick = rng.permutation(others)[:hub_deg]
        W[hub, pick] = rng.uniform(0.15, 1.0, size=len(pick))
    W = np.triu(np.maximum(W, W.T), 1)                            # one weight per pair, no diagonal
    W = W + W.T
    return normalised(W)


def normalised(W):
    """the CSR of a dense symmetric matrix of non-negative weights, scaled to sum 1 and stored as f32"""
    W32 = (W / W.sum()).astype(np.float32)
    rows, col = np.nonzero(W32)
    rowptr = np.concatenate([[0], np.cumsum((W32 > 0).sum(axis=1))]).astype(np.int64)
    return rowptr, col.astype(np.int32), W32[rows, col]


def rescaled(rowptr, col, w):
    """a CSR with the same pattern whose f32 weights sum to 1 (w / sum w)"""
    w = np.asarray(w, dtype=np.float64)
    return rowptr, col, (w / w.sum()).astype(np.float32)
