"""The inputs of chain A's tests, shared by tests/test_anchor_cases.py, which checks on the CPU that the
restatement has the chain's properties on them and that they are sharp where labels are compared, and
tests/test_gpu_anchors.py, which holds the kernels to the restatement.  TEST INFRASTRUCTURE ONLY.

Every case is a dict: Xr (n, dim), Xq (m, dim), kw = find_transfer_anchors' keywords, and what the case plants.  `found(name)`
and `weighted(name, k_weight, sd_weight)` run the restatement once per session and leave the arrays read-only."""
import functools

import numpy as np

import anchor_reference as aref


def blobs(n, m, dim, nb, seed, spread=0.6, sep=4.0):
    """nb separated Gaussian blobs, reference and query cells drawn from the same centres -> (Xr, Xq, blob of each)"""
    rng = np.random.default_rng(seed)
    cen = rng.normal(size=(nb, dim)) * sep
    lr, lq = rng.integers(0, nb, n), rng.integers(0, nb, m)
    Xr = (cen[lr] + rng.normal(size=(n, dim)) * spread).astype(np.float32)
    Xq = (cen[lq] + rng.normal(size=(m, dim)) * spread).astype(np.float32)
    return Xr, Xq, lr, lq


def _blobs4():
    Xr, Xq, lr, lq = blobs(300, 200, 10, 4, 1)
    return dict(Xr=Xr, Xq=Xq, kw=dict(k_anchor=5, k_score=30), blob_ref=lr, blob_query=lq)


def _dim1():
    # one coordinate: l2_norm would leave only +-1, so the raw coordinates are searched
    rng = np.random.default_rng(2)
    return dict(Xr=rng.uniform(-1, 1, size=(120, 1)).astype(np.float32), Xq=rng.uniform(-1, 1, size=(90, 1)).astype(np.float32),
                kw=dict(k_anchor=5, k_score=10, l2_norm=False))


def _dim64():
    Xr, Xq, lr, lq = blobs(150, 130, 64, 3, 3, spread=1.0, sep=1.5)
    return dict(Xr=Xr, Xq=Xq, kw=dict(k_anchor=5, k_score=20), blob_ref=lr, blob_query=lq)


def _kmin():
    # K = k_score = m = min(n, m): every QQ row and every RQ row holds ALL query cells
    Xr, Xq, lr, lq = blobs(40, 33, 6, 2, 4)
    return dict(Xr=Xr, Xq=Xq, kw=dict(k_anchor=5, k_score=33), blob_ref=lr, blob_query=lq)


def _ka_eq_ks():
    Xr, Xq, lr, lq = blobs(100, 80, 5, 3, 5)
    return dict(Xr=Xr, Xq=Xq, kw=dict(k_anchor=7, k_score=7), blob_ref=lr, blob_query=lq)


def _copy():
    # five isolated clusters of 12 cells; the query IS the reference: (i, i) is at distance 0 and mutual, its two cells have the
    # same four neighbour lists, so raw = 2 k_score
    rng = np.random.default_rng(6)
    cen = rng.normal(size=(5, 8)) * 6.0
    Xr = (np.repeat(cen, 12, axis=0) + rng.normal(size=(60, 8)) * 0.3).astype(np.float32)
    return dict(Xr=Xr, Xq=Xr.copy(), kw=dict(k_anchor=5, k_score=10), blob_ref=np.repeat(np.arange(5), 12),
                blob_query=np.repeat(np.arange(5), 12))


def _hole():
    # reference cell 40 lies far from everything (no query cell lists it: zero anchors); query cells 0 and 1 sit almost on the
    # first and the last reference cell (mutual first neighbours): both ends of the scan carry anchors
    rng = np.random.default_rng(7)
    Xr = rng.normal(size=(80, 4)).astype(np.float32)
    Xq = rng.normal(size=(70, 4)).astype(np.float32)
    Xr[40] = 100.0
    Xq[0], Xq[1] = Xr[0] + np.float32(1e-3), Xr[79] + np.float32(1e-3)
    return dict(Xr=Xr, Xq=Xq, kw=dict(k_anchor=5, k_score=10, l2_norm=False))


def _dk0():
    # 20 reference cells around P; query cells 0..29 ARE P, the 20 others lie 3 to 5 away.  Every reference cell's five nearest
    # query cells are copies 0..4 (equal distances: the index decides), so U = {0..4}, all one point: with k_weight = 5 a copy of
    # P has dk = 0 (ratio 0, t = score) and every other query cell sees five equal distances (ratio 1, t = 0: a zero row)
    rng = np.random.default_rng(8)
    P = np.array([1.0, 2.0, -1.0], dtype=np.float32)
    Xr = (P + rng.normal(size=(20, 3)) * 0.1).astype(np.float32)
    far = rng.normal(size=(20, 3))
    far = far / np.linalg.norm(far, axis=1)[:, None] * rng.uniform(3, 5, size=(20, 1))
    Xq = np.concatenate([np.tile(P, (30, 1)), (P + far).astype(np.float32)]).astype(np.float32)
    return dict(Xr=Xr, Xq=Xq, kw=dict(k_anchor=5, k_score=10, l2_norm=False), k_weight=5)


def _equal_raw():
    # n = m = K = k_score: every list holds every cell, raw = 2 k_score for every anchor, hi == lo, every score is 1
    rng = np.random.default_rng(9)
    return dict(Xr=rng.normal(size=(6, 3)).astype(np.float32), Xq=rng.normal(size=(6, 3)).astype(np.float32),
                kw=dict(k_anchor=3, k_score=6))


def _tie():
    # six sites 10 apart on the x axis: query cell s at (10 s, 0), reference cells 2 s at (10 s, +1) (class 0) and 2 s + 1 at
    # (10 s, -1) (class 1).  With k_anchor = k_score = 2 every query cell has exactly those two anchors, mirror images of each
    # other with the same raw score, so both classes collect the same weights in the same order: an exact tie everywhere
    s = np.arange(6, dtype=np.float32) * 10.0
    Xq = np.stack([s, np.zeros(6, dtype=np.float32)], axis=1)
    Xr = np.stack([np.repeat(s, 2), np.tile(np.array([1.0, -1.0], dtype=np.float32), 6)], axis=1)
    return dict(Xr=Xr.astype(np.float32), Xq=Xq.astype(np.float32), kw=dict(k_anchor=2, k_score=2, l2_norm=False),
                labels=np.tile(np.array([11, 4]), 6), k_weight=3)


def _big():
    # more than 65 536 anchors: the scan runs past one 1024-cell tile many times over and the fills past one grid of 256-thread
    # workgroups.  The query is the shuffled reference plus noise.  The restatement's kNN would take minutes here: the GPU test
    # checks sampled rows of the device's tables and feeds them to A2 / A3 of the restatement
    rng = np.random.default_rng(5)
    Xr = rng.normal(size=(20000, 4)).astype(np.float32)
    Xq = (Xr[rng.permutation(20000)] + rng.normal(size=(20000, 4)).astype(np.float32) * np.float32(0.05)).astype(np.float32)
    return dict(Xr=Xr, Xq=Xq, kw=dict(k_anchor=5, k_score=5, l2_norm=False))


def _subsample():
    # the sub-sampling flow's shape: 2638 cells in 15 dimensions, 1000 kept (the reference), the others mapped onto them
    rng = np.random.default_rng(10)
    cen = rng.normal(size=(6, 15)) * 3.0
    lab = rng.integers(0, 6, 2638)
    X = (cen[lab] + rng.normal(size=(2638, 15))).astype(np.float32)
    kept = np.sort(rng.choice(2638, 1000, replace=False))
    held = np.setdiff1d(np.arange(2638), kept)
    return dict(Xr=X[kept], Xq=X[held], kw=dict(k_anchor=5, k_score=30), blob_ref=lab[kept], blob_query=lab[held])


BUILDERS = dict(blobs4=_blobs4, dim1=_dim1, dim64=_dim64, kmin=_kmin, ka_eq_ks=_ka_eq_ks, copy=_copy, hole=_hole, dk0=_dk0,
                equal_raw=_equal_raw, tie=_tie, big=_big, subsample=_subsample)
SMALL = [name for name in BUILDERS if name not in ("big", "subsample")]        # the restatement runs whole on these


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def case(name):
    return _freeze(BUILDERS[name]())


@functools.lru_cache(maxsize=None)
def found(name):
    c = case(name)
    return _freeze(aref.find_anchors(c["Xq"], c["Xr"], **c["kw"]))


@functools.lru_cache(maxsize=None)
def weighted(name, k_weight, sd_weight=1.0):
    return _freeze(aref.weights(found(name), k_weight, sd_weight))


def n_anchor_queries(name):
    return len(found(name)["U"])


# (case, k_weight, sd_weight): k_weight = |U| exactly (kmin, dk0, equal_raw: asserted in test_anchor_cases.py), k_weight = 64,
# both other sd_weight, dk = 0 and zero rows (dk0), hi == lo (equal_raw)
WEIGHT_CASES = [("blobs4", 50, 1.0), ("blobs4", 64, 1.0), ("blobs4", 50, 0.5), ("blobs4", 20, 2.0), ("kmin", None, 1.0),
                ("dk0", 5, 1.0), ("equal_raw", None, 1.0), ("copy", 30, 1.0), ("dim64", 50, 1.0)]


def weight_case(name, k_weight, sd_weight):
    """k_weight None: |U|"""
    return name, n_anchor_queries(name) if k_weight is None else k_weight, sd_weight


# ---- label sets on blobs4 (n = 300, four planted blobs) ----------------------------------------------------------------------------

def label_sets():
    """name -> (labels of the 300 reference cells of blobs4, whether label equality is asserted outside the near-tie set)"""
    blob = case("blobs4")["blob_ref"]
    rng = np.random.default_rng(20)
    planted = blob.astype(np.int64).copy()
    planted[rng.choice(300, 60, replace=False)] = -1                          # unlabelled reference cells
    odd = np.array([7, -3, 1000, 7])[blob]                                    # blob 1 is unlabelled (-3); values come back as given
    return dict(planted=planted, odd_values=odd, one_class=np.full(300, 5), own_class=np.arange(300) + 10)
