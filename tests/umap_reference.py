"""numpy restatement of chain U (kernels: csrc/umap_kernels.hip), the role tests/prep_reference.py plays
for preprocessing.  TEST INFRASTRUCTURE ONLY: nothing in the package imports it.

Every stage in fp64; U4 also in float32, operation for operation as the specification writes it (sequential sum over a
vertex's terms: entry by entry, attraction then negatives); a numpy Philox-4x32-10 for the negatives."""
import numpy as np

PH_M0, PH_M1 = 0xD2511F53, 0xCD9E8D57
PH_W0, PH_W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Four uint32 arrays: the Philox-4x32-10 block of every counter (c0..c3 broadcast) under the key (k0, k1)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(PH_M0) * c0, np.uint64(PH_M1) * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(PH_W0)) & MASK, (k1 + np.uint64(PH_W1)) & MASK
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


# ---- U1 -----------------------------------------------------------------------------------------------------------------------

def normalize_rows(X):
    """cosine's host step: fp64 sum of squares in coordinate order, sqrt, fp64 quotient rounded to f32; zero rows stay zero"""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    ss = np.zeros(len(X64))
    for c in range(X64.shape[1]):
        ss = ss + X64[:, c] * X64[:, c]
    nrm = np.sqrt(ss)
    out = np.zeros_like(X64)
    ok = nrm > 0
    out[ok] = X64[ok] / nrm[ok, None]
    return out.astype(np.float32)


def knn_exact(X, k):
    """(n, k) indices by brute force in fp64: column 0 the point, then ascending (d2, index) -- for CPU-only reference runs
    (the device ranks by its f32 chain: the two can order a near-tie differently)"""
    X = np.asarray(X, dtype=np.float64)
    n = len(X)
    nn = np.empty((n, k), dtype=np.int32)
    for r0 in range(0, n, 256):                                               # (row blocks: memory)
        rows = np.arange(r0, min(r0 + 256, n))
        d2 = ((X[rows, None, :] - X[None, :, :]) ** 2).sum(axis=2)
        d2[np.arange(len(rows)), rows] = -1.0
        nn[rows] = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return nn


def distances(X, nn, metric):
    """U1's distances of the given indices (X: the f32 points; for cosine the UNIT rows): the f32 fmaf chain over the coordinates in
    ascending order, every fmaf evaluated in fp64 (the square of an f32 difference is exact there) and rounded to f32, then
    sqrtf, or d2 / 2 for cosine.  The fp64 sum is rounded once more when it becomes f32: a chain step can differ from the
    fused one by one f32 step on a rare tie."""
    X = np.asarray(X, dtype=np.float32)
    nn = np.asarray(nn)
    d = np.zeros(nn.shape, dtype=np.float32)
    for c in range(X.shape[1]):
        df = (X[:, c][:, None] - X[:, c][nn]).astype(np.float32)            # f32 subtraction
        d = (d.astype(np.float64) + df.astype(np.float64) * df.astype(np.float64)).astype(np.float32)
    return d * np.float32(0.5) if metric == "cosine" else np.sqrt(d)         # (np.sqrt of f32 is correctly rounded)


# ---- U2 -----------------------------------------------------------------------------------------------------------------------

def smooth(dist):
    """(rho, sigma, floor_binds, mean_i): fp64, exactly 64 bisection steps, no early exit"""
    d = np.asarray(dist, dtype=np.float32).astype(np.float64)
    n, k = d.shape
    pos = np.where((d > 0) & (np.arange(k)[None, :] >= 1), d, np.inf)
    rho = pos.min(axis=1)
    rho = np.where(np.isinf(rho), 0.0, rho)
    mean_i = np.zeros(n)
    for p in range(k):
        mean_i = mean_i + d[:, p]
    mean_i = mean_i / k
    mean_all = (np.cumsum(mean_i)[-1]) / n                                    # cumsum: index order
    target = np.log2(float(k))
    x = d[:, 1:] - rho[:, None]
    lo, hi, mid = np.zeros(n), np.full(n, np.inf), np.ones(n)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for _ in range(64):
            psum = np.zeros(n)
            for p in range(k - 1):
                psum = psum + np.where(x[:, p] > 0, np.exp(-(x[:, p] / mid)), 1.0)
            up = psum > target
            hi = np.where(up, mid, hi)
            lo = np.where(up, lo, mid)
            mid = np.where(up, (lo + hi) / 2.0, np.where(np.isinf(hi), 2.0 * mid, (lo + hi) / 2.0))
    floor_ = 1e-3 * np.where(rho > 0, mean_i, mean_all)
    return rho, np.maximum(mid, floor_), floor_ >= mid, mean_i


# ---- U3 -----------------------------------------------------------------------------------------------------------------------

def union(nn, dist, rho, sigma):
    """(rowptr, col, w64, w32): dense n x n in fp64 (test sizes only); entries whose f32 weight is 0 are dropped"""
    nn = np.asarray(nn)
    d = np.asarray(dist, dtype=np.float32).astype(np.float64)
    n, k = nn.shape
    V = np.zeros((n, n))
    x = d[:, 1:] - rho[:, None]
    with np.errstate(under="ignore", over="ignore"):
        v = np.where(x <= 0, 1.0, np.exp(-(x / sigma[:, None])))
    V[np.repeat(np.arange(n), k - 1), nn[:, 1:].ravel()] = v.ravel()
    W = V + V.T - V * V.T
    W32 = W.astype(np.float32)
    keep = W32 > 0
    keep[np.arange(n), np.arange(n)] = False
    rowptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    rows, col = np.nonzero(keep)                                              # row-major: rows ascending by column
    return rowptr, col.astype(np.int32), W[rows, col], W32[rows, col]


# ---- U4 -----------------------------------------------------------------------------------------------------------------------

def fire_counts(p, T):
    """how often an edge of ratio p (f32) fires in T epochs, by the specification's f32 test"""
    p = np.float32(p)
    return sum(int(np.floor(np.float32(t + 1) * p)) - int(np.floor(np.float32(t) * p)) >= 1 for t in range(T))


# One deliberate deviation each, named after the line of k_umap_layout it stands for; tests/test_umap_host.py shows that the
# small-step criterion of the GPU tests sees every one of them.
MUTATIONS = (
    "philox_t_q",       # philox4x32_10(v, E, t, q): the counter words t and q exchanged
    "philox_local_E",   # ... E the entry's index within its row (E - rowptr[v]) instead of the global CSR index
    "fire_next",        # floorf(tf1 * pe) - floorf(tf0 * pe): the firing test of epoch t + 1
    "alpha_next",       # alpha: the host passes the step of epoch t + 1
    "keep_self",        # if (j == v) continue: the draw is not skipped (s = 0: it takes the +4 rule)
    "no_eps",           # (0.001f + s): 0.001 left out of the repulsive denominator
    "clamp_coef",       # clamp4(coef * d[c]): the clamp applied to the coefficient, clamp4(coef) * d[c]
)


def layout(rowptr, col, w, Y0, a, b, alpha0, T, neg, seed, dtype=np.float64, mutate=None):
    """U4 in `dtype` arithmetic.  The schedule (p_e, the firing test, alpha_t) is the specification's f32 / fp64 mix in both;
    a, b, alpha0 are taken as f32 values.  A vertex's terms are added one by one in the specification's order.
    `mutate`: None (the specification), or one of MUTATIONS: the specification with that one line wrong."""
    assert mutate is None or mutate in MUTATIONS, mutate
    dt = np.dtype(dtype).type
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    w = np.asarray(w, dtype=np.float32)
    Y = np.array(Y0, dtype=np.float32).astype(dt)
    n, c = Y.shape
    nnz = len(col)
    if nnz == 0:
        return Y
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    nonempty = np.diff(rowptr) > 0
    p = (w / w.max()).astype(np.float32)
    a, b = dt(np.float32(a)), dt(np.float32(b))
    m2ab, twob, bm1 = dt(-2.0) * a * b, dt(2.0) * b, b - dt(1.0)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    E_all = np.arange(nnz, dtype=np.int64)
    eps = dt(0.0) if mutate == "no_eps" else dt(0.001)

    def force(coef, d):
        if mutate == "clamp_coef":
            return np.clip(coef, dt(-4.0), dt(4.0))[..., None] * d
        return np.clip(coef[..., None] * d, dt(-4.0), dt(4.0))

    def sq(d):
        s = d[..., 0] * d[..., 0]
        for q in range(1, c):
            s = s + d[..., q] * d[..., q]
        return s

    qs = np.arange(neg, dtype=np.int64)[None, :]
    for t in range(T):
        ta, tf = t + (mutate == "alpha_next"), t + (mutate == "fire_next")
        alpha = dt(np.float32(float(np.float32(alpha0)) * (1.0 - float(ta) / float(T))))
        fire = (np.floor(np.float32(tf + 1) * p).astype(np.int64) - np.floor(np.float32(tf) * p).astype(np.int64)) >= 1
        E = E_all[fire]
        i, j = rows[E], col[E]
        terms = np.zeros((len(E), 1 + neg, c), dtype=dt)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            d = Y[i] - Y[j]
            s = sq(d)
            ok = s > 0
            ss = np.where(ok, s, dt(1.0))
            coef = (m2ab * np.power(ss, bm1)) / (a * np.power(ss, b) + dt(1.0))
            terms[:, 0, :] = np.where(ok[:, None], force(coef, d), dt(0.0))
            if neg:
                Ec = (E - rowptr[i] if mutate == "philox_local_E" else E)[:, None]
                ctr = (i[:, None], Ec, qs, t) if mutate == "philox_t_q" else (i[:, None], Ec, t, qs)
                jn = (philox4x32_10(*ctr, k0, k1)[0] % np.uint32(n)).astype(np.int64)
                d = Y[i][:, None, :] - Y[jn]
                s = sq(d)
                ok = s > 0
                ss = np.where(ok, s, dt(1.0))
                coef = twob / ((eps + ss) * (a * np.power(ss, b) + dt(1.0)))
                term = np.where(ok[..., None], force(coef, d), dt(4.0))
                terms[:, 1:, :] = term if mutate == "keep_self" else np.where((jn == i[:, None])[..., None], dt(0.0), term)
        g = np.zeros((n, c), dtype=dt)
        np.add.at(g, np.repeat(i, 1 + neg), terms.reshape(-1, c))            # unbuffered: one term after the other
        Y = np.where(nonempty[:, None], Y + alpha * g, Y)
        assert Y.dtype == np.dtype(dtype)
    return Y


# ---- quality -------------------------------------------------------------------------------------------------------------------

def knn_preservation(nn_high, Y, k=None):
    nn_high = np.asarray(nn_high)
    k = nn_high.shape[1] if k is None else k
    nn_low = knn_exact(Y, k)
    return float((nn_high[:, 1:k, None] == nn_low[:, None, 1:]).any(axis=2).mean())


def label_purity(Y, labels, k=16):
    """fraction of the k - 1 nearest embedding neighbours of a point that carry its label, averaged"""
    nn_low = knn_exact(Y, k)
    labels = np.asarray(labels)
    return float((labels[nn_low[:, 1:]] == labels[:, None]).mean())


def blobs(seed=0, n=600, dim=10, sep=10.0):
    """three unit-variance Gaussian blobs whose centres are `sep` apart and not collinear (an equilateral triangle)"""
    rng = np.random.default_rng(seed)
    centres = np.zeros((3, dim))
    centres[1, 0] = sep
    centres[2, 0], centres[2, 1] = sep / 2.0, sep * np.sqrt(3.0) / 2.0
    labels = np.arange(n) % 3
    return (centres[labels] + rng.normal(size=(n, dim))).astype(np.float32), labels


def reference_graph(X, k, metric="euclidean"):
    """U1 - U3 on the CPU -> (nn, rowptr, col, w32)"""
    Xs = normalize_rows(X) if metric == "cosine" else np.asarray(X, dtype=np.float32)
    nn = knn_exact(Xs, k)
    dist = distances(Xs, nn, metric)
    rho, sigma, _, _ = smooth(dist)
    rowptr, col, _, w32 = union(nn, dist, rho, sigma)
    return nn, rowptr, col, w32


def handmade_graph(n=203, hub=7, hub_deg=130, lonely=50, tiny=(3, 4), T=8, seed=0):
    """A symmetric CSR for the layout tests: a ring over all vertices but `lonely` (an empty row) and n - 1; vertex `hub`
    joined to hub_deg vertices in all; weights spread over (0, 1], the largest exactly 1; two edges whose weight 0.9 / T is
    below 1 / T (they never fire in T epochs): the ring edge `tiny`, and {n - 2, n - 1}, the only edge of vertex n - 1 and the
    last entry of the CSR in both directions (removing it renumbers no other entry).  n is no multiple of 64."""
    rng = np.random.default_rng(seed)
    W = np.zeros((n, n))
    ring = [v for v in range(n - 1) if v != lonely]
    for x, y in zip(ring, ring[1:] + ring[:1]):
        W[x, y] = W[y, x] = rng.uniform(0.15, 1.0)
    others = [v for v in range(n - 1) if v not in (hub, lonely) and W[hub, v] == 0]
    for v in rng.permutation(others)[:hub_deg - int((W[hub] > 0).sum())]:
        W[hub, v] = W[v, hub] = rng.uniform(0.15, 1.0)
    W[ring[0], ring[1]] = W[ring[1], ring[0]] = 1.0
    W[tiny[0], tiny[1]] = W[tiny[1], tiny[0]] = 0.9 / T
    W[n - 2, n - 1] = W[n - 1, n - 2] = 0.9 / T
    W32 = W.astype(np.float32)
    rows, col = np.nonzero(W32)
    rowptr = np.concatenate([[0], np.cumsum((W32 > 0).sum(axis=1))]).astype(np.int64)
    return rowptr, col.astype(np.int32), W32[rows, col]


def drop_edge(rowptr, col, w, x, y):
    """the same CSR without the edge {x, y}"""
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    keep = ~(((rows == x) & (col == y)) | ((rows == y) & (col == x)))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=len(rowptr) - 1))]).astype(np.int64)
    return rp, col[keep], w[keep]


def random_graph(n, density, seed):
    """a symmetric CSR with about density * (n - 1) entries per row, weights U(0.15, 1], the largest exactly 1"""
    rng = np.random.default_rng(seed)
    U = np.triu(rng.uniform(0.15, 1.0, size=(n, n)) * (rng.random((n, n)) < density), 1)
    U[np.unravel_index(np.argmax(U), U.shape)] = 1.0
    W32 = (U + U.T).astype(np.float32)
    rows, col = np.nonzero(W32)
    rowptr = np.concatenate([[0], np.cumsum((W32 > 0).sum(axis=1))]).astype(np.int64)
    return rowptr, col.astype(np.int32), W32[rows, col]


def degree_graph(n, nnz, empty=(), hub=None, hub_deg=0, seed=0):
    """A CSR of exactly `nnz` entries (mean row length nnz / n, any rational with denominator n): the rows in `empty` hold
    nothing, the others form a ring; vertex `hub` is joined to hub_deg vertices in all; random pairs fill up to nnz // 2
    edges, stored both ways with one weight U(0.15, 1), the largest weight exactly 1.  A symmetric CSR without a diagonal has
    an even number of entries: an odd nnz adds ONE entry x -> y without its mirror (mi_umap_layout_f32 uses the rows as
    given; symmetry is the caller's business)."""
    rng = np.random.default_rng(seed)
    live = [v for v in range(n) if v not in set(empty)]
    W = np.zeros((n, n))
    for x, y in zip(live, live[1:] + live[:1]):
        W[x, y] = W[y, x] = rng.uniform(0.15, 1.0)
    if hub is not None:
        others = [v for v in live if v != hub and W[hub, v] == 0]
        for v in rng.permutation(others)[:hub_deg - int((W[hub] > 0).sum())]:
            W[hub, v] = W[v, hub] = rng.uniform(0.15, 1.0)
    free = [(x, y) for x in live for y in live if x < y and W[x, y] == 0]
    free = [free[q] for q in rng.permutation(len(free))]
    more = nnz // 2 - int((W > 0).sum()) // 2
    assert 0 <= more and more + (nnz & 1) <= len(free), "nnz = %d does not fit" % nnz
    for x, y in free[:more]:
        W[x, y] = W[y, x] = rng.uniform(0.15, 1.0)
    if nnz & 1:
        W[free[more]] = rng.uniform(0.15, 1.0)
    W[live[0], live[1]] = W[live[1], live[0]] = 1.0
    W32 = W.astype(np.float32)
    rows, col = np.nonzero(W32)
    rowptr = np.concatenate([[0], np.cumsum((W32 > 0).sum(axis=1))]).astype(np.int64)
    return rowptr, col.astype(np.int32), W32[rows, col]


def schedule_graph(T):
    """Eight vertices on a path (plus the chord {0, 5}) whose weights are the firing ratios themselves (the largest is 1):
    1, one f32 step below 1, float32(1/3), float32(2/3), float32(1/T), 1/2, 1/4 and, on {6, 7}, one f32 step below
    float32(1/T), which never fires in T epochs.  {6, 7} is the only edge of vertex 7 and the last entry of the CSR in both
    directions: removing it renumbers no other entry.  -> (rowptr, col, w, {edge: weight})"""
    one, inv = np.float32(1.0), np.float32(1.0) / np.float32(T)
    edges = {(0, 1): one, (1, 2): np.nextafter(one, np.float32(0.0)), (2, 3): np.float32(1.0 / 3.0),
             (3, 4): np.float32(2.0 / 3.0), (4, 5): inv, (5, 6): np.float32(0.5), (0, 5): np.float32(0.25),
             (6, 7): np.nextafter(inv, np.float32(0.0))}
    W32 = np.zeros((8, 8), dtype=np.float32)
    for (x, y), v in edges.items():
        W32[x, y] = W32[y, x] = v
    rows, col = np.nonzero(W32)
    rowptr = np.concatenate([[0], np.cumsum((W32 > 0).sum(axis=1))]).astype(np.int64)
    return rowptr, col.astype(np.int32), W32[rows, col], edges
