"""numpy restatement of chain Q (kernels: csrc/mapping_kernels.hip): mapping new points onto a fixed
reference.  TEST INFRASTRUCTURE ONLY: nothing in the package imports it.

Q1 ranks by the f32 chain of umap_reference.distances; Q2, Q3 and Q5 are fp64 in column order; Q4 in fp64 and in float32,
operation for operation as the specification writes it (a query's terms one after the other: entry by entry, attraction
then negatives), with umap_reference's Philox."""
import numpy as np

import umap_reference as ref

normalize_rows = ref.normalize_rows


# ---- Q1 -----------------------------------------------------------------------------------------------------------------------

def chain_d2(Q, R, nn):
    """the f32 fmaf chain of (query i, reference nn[i, p]) over the coordinates in ascending order, df = q_c - r_c: the loop of
    umap_reference.distances with the two sets apart (every fmaf evaluated in fp64 and rounded to f32)"""
    Q, R = np.asarray(Q, dtype=np.float32), np.asarray(R, dtype=np.float32)
    nn = np.asarray(nn)
    d = np.zeros(nn.shape, dtype=np.float32)
    for c in range(Q.shape[1]):
        df = (Q[:, c][:, None] - R[:, c][nn]).astype(np.float32)
        d = (d.astype(np.float64) + df.astype(np.float64) * df.astype(np.float64)).astype(np.float32)
    return d


def distances(Q, R, nn, metric):
    """Q1's distances of the given indices (for cosine: the UNIT rows of both sets)"""
    d = chain_d2(Q, R, nn)
    return d * np.float32(0.5) if metric == "cosine" else np.sqrt(d)


def cross_knn(Q, R, k):
    """(m, k) indices into R by ascending (chain d2, index); nothing excluded"""
    R = np.asarray(R, dtype=np.float32)
    m, n = len(Q), len(R)
    d2 = chain_d2(Q, R, np.broadcast_to(np.arange(n), (m, n)))
    return np.argsort(d2, axis=1, kind="stable")[:, :k].astype(np.int32)


# ---- Q2 -----------------------------------------------------------------------------------------------------------------------

def smooth(dist):
    """(sigma, w32, floor_binds): rho = 0, the sum over ALL k columns, the floor from the row's own mean; fp64, exactly 64
    bisection steps; the weights in fp64, stored as f32"""
    d = np.asarray(dist, dtype=np.float32).astype(np.float64)
    m, k = d.shape
    mean_i = np.zeros(m)
    for p in range(k):
        mean_i = mean_i + d[:, p]
    mean_i = mean_i / k
    target = np.log2(float(k))
    lo, hi, mid = np.zeros(m), np.full(m, np.inf), np.ones(m)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for _ in range(64):
            psum = np.zeros(m)
            for p in range(k):
                psum = psum + np.where(d[:, p] > 0, np.exp(-(d[:, p] / mid)), 1.0)
            up = psum > target
            hi = np.where(up, mid, hi)
            lo = np.where(up, lo, mid)
            mid = np.where(up, (lo + hi) / 2.0, np.where(np.isinf(hi), 2.0 * mid, (lo + hi) / 2.0))
    floor_ = 1e-3 * mean_i
    sigma = np.where(mid > floor_, mid, floor_)
    return sigma, weights(dist, sigma), floor_ >= mid


def weights(dist, sigma):
    """v_ip = (d_ip > 0 ? exp(-d_ip / sigma_i) : 1) in fp64, stored as f32"""
    d = np.asarray(dist, dtype=np.float32).astype(np.float64)
    with np.errstate(over="ignore", under="ignore"):
        return np.where(d > 0, np.exp(-(d / np.asarray(sigma)[:, None])), 1.0).astype(np.float32)


# ---- Q3 -----------------------------------------------------------------------------------------------------------------------

def init(nn, w, Yref):
    """the weighted mean of the neighbours' positions: fp64 in column order on the stored f32 weights, rounded to f32"""
    nn = np.asarray(nn)
    w = np.asarray(w, dtype=np.float32).astype(np.float64)
    Y = np.asarray(Yref, dtype=np.float32).astype(np.float64)
    num, den = np.zeros((len(nn), Y.shape[1])), np.zeros(len(nn))
    for p in range(nn.shape[1]):
        num = num + w[:, p][:, None] * Y[nn[:, p]]
        den = den + w[:, p]
    return (num / den[:, None]).astype(np.float32)


# ---- Q5 -----------------------------------------------------------------------------------------------------------------------

def vote(nn, u, labels, L):
    """(label, score, scores): u = the (m, k) weights of the vote (ones for the uniform one), labels -1 or in [0, L).  Shares of
    the labelled neighbours' total in fp64, column order; the largest wins, ties to the smaller label; a row whose labelled
    neighbours weigh nothing gets -1 and 0."""
    nn = np.asarray(nn)
    u = np.asarray(u, dtype=np.float64)
    lab = np.asarray(labels)[nn]
    m, k = nn.shape
    scores = np.zeros((m, L))
    label, score = np.full(m, -1, dtype=np.int32), np.zeros(m)
    for i in range(m):
        total, sums = 0.0, {}
        for p in range(k):
            if lab[i, p] >= 0:
                total += u[i, p]
                sums[int(lab[i, p])] = sums.get(int(lab[i, p]), 0.0) + u[i, p]
        if total > 0.0:
            for l in sorted(sums):
                scores[i, l] = sums[l] / total
                if scores[i, l] > score[i] or label[i] < 0:
                    label[i], score[i] = l, scores[i, l]
    return label, score, scores


# ---- Q4 -----------------------------------------------------------------------------------------------------------------------

# One deliberate deviation each; tests/test_mapping_host.py shows that the small-step criterion of the GPU tests sees every one.
MUTATIONS = (
    "philox_t_q",        # philox4x32_10(q0 + v, gl, t, q): the counter words t and q exchanged
    "no_q0",             # ... q0 ignored: the query's index within its call
    "mod_m",             # r[0] % n: the draw taken modulo the number of queries
    "neg_from_queries",  # load_y(Yref, j): the negative's position read from the queries' (row j modulo m of the moving points)
    "keep_skip",         # U4's `if (j == v) continue` kept, although j is a reference index and v a query's
    "batch_max",         # w / (the row's largest weight): divided by the largest weight of the whole call
    "fire_next",         # the firing test of epoch t + 1
    "alpha_next",        # alpha[t]: the step of epoch t + 1
)


def ratios(w, mutate=None):
    """p_ip = w_ip / (the ROW's largest weight), one f32 division"""
    w = np.asarray(w, dtype=np.float32)
    top = w.max() if mutate == "batch_max" else w.max(axis=1, keepdims=True)
    return (w / top).astype(np.float32)


def layout(nn, w, Yref, Y0, a, b, alpha0, T, neg, seed, q0=0, dtype=np.float64, mutate=None):
    """Q4 in `dtype` arithmetic; the schedule (ratios, the firing test, alpha_t) is the specification's f32 / fp64 mix in both;
    a, b, alpha0 are taken as f32 values.  `mutate`: None (the specification) or one of MUTATIONS."""
    assert mutate is None or mutate in MUTATIONS, mutate
    dt = np.dtype(dtype).type
    nn = np.asarray(nn, dtype=np.int64)
    Yr = np.asarray(Yref, dtype=np.float32).astype(dt)
    Y = np.array(Y0, dtype=np.float32).astype(dt)
    (m, k), (n, c) = nn.shape, Yr.shape
    p = ratios(w, mutate)
    a, b = dt(np.float32(a)), dt(np.float32(b))
    m2ab, twob, bm1 = dt(-2.0) * a * b, dt(2.0) * b, b - dt(1.0)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    first = 0 if mutate == "no_q0" else int(q0)

    def force(coef, d):
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
        i, col = np.nonzero(fire)                                            # row-major: a row's entries in column order
        terms = np.zeros((len(i), 1 + neg, c), dtype=dt)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            d = Y[i] - Yr[nn[i, col]]
            s = sq(d)
            ok = s > 0
            ss = np.where(ok, s, dt(1.0))
            coef = (m2ab * np.power(ss, bm1)) / (a * np.power(ss, b) + dt(1.0))
            terms[:, 0, :] = np.where(ok[:, None], force(coef, d), dt(0.0))
            if neg and len(i):
                ctr = ((first + i)[:, None], col[:, None], qs, t) if mutate == "philox_t_q" else \
                      ((first + i)[:, None], col[:, None], t, qs)
                r = ref.philox4x32_10(*ctr, k0, k1)[0]
                jn = (r % np.uint32(m if mutate == "mod_m" else n)).astype(np.int64)
                yj = Y[jn % m] if mutate == "neg_from_queries" else Yr[jn % n]     # (% n: only "mod_m" with m > n needs it)
                d = Y[i][:, None, :] - yj
                s = sq(d)
                ok = s > 0
                ss = np.where(ok, s, dt(1.0))
                coef = twob / ((dt(0.001) + ss) * (a * np.power(ss, b) + dt(1.0)))
                term = np.where(ok[..., None], force(coef, d), dt(4.0))
                terms[:, 1:, :] = np.where((jn == i[:, None])[..., None], dt(0.0), term) if mutate == "keep_skip" else term
        g = np.zeros((m, c), dtype=dt)
        np.add.at(g, np.repeat(i, 1 + neg), terms.reshape(-1, c))            # unbuffered: one term after the other
        Y = Y + alpha * g
        assert Y.dtype == np.dtype(dtype)
    return Y


def draws(i, p, t, neg, n, seed, q0=0):
    """the `neg` reference indices entry p of query q0 + i draws at epoch t"""
    r = ref.philox4x32_10(int(q0) + int(i), int(p), int(t), np.arange(neg), int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)[0]
    return (r % np.uint32(n)).astype(np.int64)


def transform(Q, R, Yref, k, metric, a, b, alpha0, T, neg, seed, q0=0, dtype=np.float64):
    """Q1 - Q4 on the CPU -> dict(nn, dist, sigma, w, init, coords)"""
    Qs, Rs = (normalize_rows(Q), normalize_rows(R)) if metric == "cosine" else (np.asarray(Q, np.float32), np.asarray(R, np.float32))
    nn = cross_knn(Qs, Rs, k)
    dist = distances(Qs, Rs, nn, metric)
    sigma, w, _ = smooth(dist)
    y0 = init(nn, w, Yref)
    return dict(nn=nn, dist=dist, sigma=sigma, w=w, init=y0,
                coords=layout(nn, w, Yref, y0, a, b, alpha0, T, neg, seed, q0, dtype))
