"""Input builders shared by tests/test_snn_host.py (what the oracle says about them, no GPU) and
tests/test_gpu_snn_edges.py (the device against the oracle on them).  Plain helpers, no fixtures."""
import numpy as np

STAR_K = 5                       # the k the star inputs are built for
ROW_CAP = 4096                   # kRowCap of csrc/snn_kernels.hip: candidates one SNN row may hold


def cloud(n, dim, seed, clusters=6):
    """Gaussian blobs on a line of centres (the generator of tests/test_gpu_snn.py)."""
    rng = np.random.RandomState(seed)
    return (rng.normal(size=(n, dim)) + 3.0 * rng.randint(0, clusters, size=(n, 1))).astype(np.float32)


def star_hub(n):
    return n // 2


def star(n, seed=1):
    """n points in 64-D of which every one lists point n // 2 (the hub) among its STAR_K - 1 nearest: random unit vectors
    (fp64 normals, normalised, cast to fp32) with the hub moved to the origin.  Every other point is at distance 1 from the
    hub and about sqrt(2) from the rest, so every pair of points shares the hub and every SNN row has exactly n - 1
    entries (tests/test_snn_host.py establishes both with the oracle at every n the GPU tests use)."""
    rng = np.random.RandomState(seed)
    V = rng.normal(size=(n, 64))
    V /= np.linalg.norm(V, axis=1, keepdims=True)
    X = V.astype(np.float32)
    X[star_hub(n)] = 0.0
    return X


def lattice(n, dim, levels, seed=0):
    """Integer coordinates in [0, levels) as fp32: few distinct points, every squared distance a small integer (exact in
    any evaluation order), so the neighbour lists are decided by the index tie-break almost everywhere."""
    rng = np.random.RandomState(seed)
    return rng.randint(0, levels, size=(n, dim)).astype(np.float32)


def chain_distances(X):
    """(n, n) fp32 squared distances by the specification's chain d = fma(x_ic - x_jc, x_ic - x_jc, d), c ascending.
    Only for inputs whose products and partial sums are exact in fp32 (the lattices): numpy has no fused multiply-add,
    and there a separate multiply and add round to the same values."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    d = np.zeros((len(X), len(X)), dtype=np.float32)
    for c in range(X.shape[1]):
        diff = X[:, None, c] - X[None, :, c]
        d = diff * diff + d
    return d


def ties_at_kth_place(X, k):
    """Per point: does the last listed neighbour (the (k - 1)-th nearest other point) tie in d with the first one left out?"""
    d = chain_distances(X)
    np.fill_diagonal(d, np.inf)
    ds = np.sort(d, axis=1)
    return ds[:, k - 2] == ds[:, k - 1]


LATTICES = [(200, 2, 3), (300, 3, 3), (130, 4, 2)]          # (n, dim, levels)
LATTICE_KS = (5, 17, 34)
STAR_SIZES = (257, 258, 513, 514, 1025, ROW_CAP + 1, ROW_CAP + 2)


def duplicates_across_tile(seed=5):
    """cloud(130, 3) with points 56 .. 71 all equal: a block of exact duplicates that straddles k_knn's tile boundary 63|64,
    longer (15 others) than k - 1 = 8 and shorter than k - 1 = 17."""
    X = cloud(130, 3, seed)
    X[56:72] = X[56]
    return X


def magnitude_cases():
    """name -> (X, k): inputs whose squared distances are subnormal, close to FLT_MAX, or dominated by cancellation."""
    tiny = (cloud(130, 3, 21).astype(np.float64) * 1e-20).astype(np.float32)
    huge = cloud(130, 1, 22)
    huge[::7] = 6e18
    huge[3::11] = -6e18                                       # range 1.2e19: S = 1.44e38 <= FLT_MAX / 2 = 1.70e38
    offset = (cloud(130, 3, 23).astype(np.float64) + 1e6).astype(np.float32)
    return {"subnormal": (tiny, 5), "near_overflow": (huge, 5), "offset_1e6": (offset, 5)}
