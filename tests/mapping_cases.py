"""The small-step cases of chain Q4 shared by tests/test_mapping_host.py, which shows on the CPU that
the criterion can see errors, and tests/test_gpu_mapping.py, which holds k_umap_transform to it.  TEST INFRASTRUCTURE ONLY.

alpha0 = 2^-10, as tests/umap_layout_cases.py: positions hardly move, every epoch's gradient is evaluated essentially at the
start, nothing amplifies, and D32 (float32 against fp64 evaluation of the restatement) falls to the storage rounding of Y.
The rows are what the chain itself makes of random points (Q1 - Q3 of the restatement): weights with rho = 0, whose row
maxima lie well below 1, and the weighted-mean start."""
import functools

import numpy as np

import mapping_reference as mref
import umap_layout_cases as uc

ALPHA0 = uc.LR
T8 = uc.T8
SEED_HI = uc.SEED_HI
AB = uc.AB["md0.1"]
SHAPES = {"m<n": (37, 67), "m>n": (83, 67)}             # (m, n): m is no multiple of 256 / G = 16, 8 or 4; n >= 64 = the largest k
GROUP = {5: 16, 16: 16, 17: 32, 32: 32, 33: 64, 64: 64}   # k -> G: every G, both sides of each threshold


def lanes(k):
    """the selection of mi_umap_transform_layout_f32: the smallest of 16, 32, 64 that holds k"""
    return 64 if k > 32 else 32 if k > 16 else 16


# (k, c, neg, seed, q0, shape): every k x c x neg; seed, q0 and shape alternate so that each G sees both values of each
CASES = []
for ki, k in enumerate(GROUP):
    for c in (2, 3):
        for ni, neg in enumerate((0, 1, 5, 16)):
            CASES.append((k, c, neg, SEED_HI if (ki + ni + c) % 2 and neg else 42, 1000 if (ni + c) % 2 else 0,
                          "m>n" if (ki // 2 + ni // 2 + c) % 2 else "m<n"))
for G in (16, 32, 64):
    mine = [case for case in CASES if GROUP[case[0]] == G and lanes(case[0]) == G]
    assert len(mine) == 16
    assert {case[3] for case in mine} == {42, SEED_HI} and {case[4] for case in mine} == {0, 1000}
    assert {case[5] for case in mine} == set(SHAPES) and {(case[1], case[2]) for case in mine} == {(c, g) for c in (2, 3) for g in (0, 1, 5, 16)}


def case_id(case):
    k, c, neg, seed, q0, shape = case
    return "k%d-c%d-neg%d-seed%s-q%d-%s" % (k, c, neg, "42" if seed == 42 else "hi", q0, shape)


@functools.lru_cache(maxsize=None)
def rows(k, c, shape):
    """(nn, w, Yref, Y0) of random points through Q1 - Q3 of the restatement, the properties the cases rely on asserted"""
    m, n = SHAPES[shape]
    rng = np.random.default_rng(1000 * k + 10 * c + m)
    R = rng.normal(size=(n, 6)).astype(np.float32)
    Q = rng.normal(size=(m, 6)).astype(np.float32)
    Yref = (rng.normal(size=(n, c)) * 4.0).astype(np.float32)
    nn = mref.cross_knn(Q, R, k)
    _, w, binds = mref.smooth(mref.distances(Q, R, nn, "euclidean"))
    Y0 = mref.init(nn, w, Yref)
    top = w.max(axis=1)
    assert not binds.any() and 0.0 < top.min() and top.max() < 0.9 and len(set(top.tolist())) > m // 2   # row maximum != batch maximum
    assert m % (256 // lanes(k)) != 0 and m != n and n >= k
    for arr in (nn, w, Yref, Y0):
        arr.setflags(write=False)
    return nn, w, Yref, Y0


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> (nn, w, Yref, Y0, y64, D32, largest move), the restatement run once per session and left unchanged"""
    k, c, neg, seed, q0, shape = case
    nn, w, Yref, Y0 = rows(k, c, shape)
    y64 = mref.layout(nn, w, Yref, Y0, *AB, ALPHA0, T8, neg, seed, q0, np.float64)
    y32 = mref.layout(nn, w, Yref, Y0, *AB, ALPHA0, T8, neg, seed, q0, np.float32)
    y64.setflags(write=False)
    return nn, w, Yref, Y0, y64, float(np.abs(y32 - y64).max()), float(np.abs(y64 - Y0).max())


# ---- handmade rows, in the manner of umap_reference.schedule_graph ------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def handmade(T, c=2, neg=1, seed=42, q0=0):
    """Six queries of k = 8 entries against n = 8 reference points whose WEIGHTS are chosen, not computed.  Every row's largest
    weight is 1/2, so the ratios are the weights doubled, exactly:
        row 0: ratios 1, one f32 step below 1, float32(1/3), float32(2/3), float32(1/T) (fires once), 1/2, 1/4 and one f32
               step below float32(1/T) (never fires in T epochs);
        row 1: the same with a stored weight of 0 in the last column;
        row 2: its start IS Yref[nn[2, 0]] (ratio 1: the attraction of epoch 0 meets s = 0 and adds nothing), and nn[2, 0] is
               the first negative that entry draws at epoch 0 (a negative on a coincident position: the +4 rule);
        rows 3 - 5: the ratios of row 0 in other orders, random starts.
    -> (nn, w, Yref, Y0, facts)"""
    one, inv = np.float32(1.0), np.float32(1.0) / np.float32(T)
    pr = np.array([one, np.nextafter(one, np.float32(0.0)), np.float32(1.0 / 3.0), np.float32(2.0 / 3.0), inv, np.float32(0.5),
                   np.float32(0.25), np.nextafter(inv, np.float32(0.0))], dtype=np.float32)
    rng = np.random.default_rng(8000 + c)
    n, m, k = 8, 6, 8
    Yref = (rng.normal(size=(n, c)) * 0.5).astype(np.float32)
    Y0 = (rng.normal(size=(m, c)) * 0.5).astype(np.float32)
    nn = np.stack([rng.permutation(n) for _ in range(m)]).astype(np.int32)
    w = np.stack([pr] + [pr] + [pr] + [pr[rng.permutation(k)] for _ in range(3)]) * np.float32(0.5)
    w[1, 7] = 0.0
    assert neg >= 1
    hit = int(mref.draws(2, 0, 0, neg, n, seed, q0)[0])
    nn[2, 0], nn[2, 1:] = hit, [j for j in range(n) if j != hit][:k - 1]
    Y0[2] = Yref[hit]
    p = mref.ratios(w)
    assert np.array_equal(p[0], pr) and np.array_equal(p[1, :7], pr[:7]) and p[1, 7] == 0.0 and (p.max(axis=1) == 1.0).all()
    return nn, w.astype(np.float32), Yref, Y0, dict(ratios=pr, hit=hit)
