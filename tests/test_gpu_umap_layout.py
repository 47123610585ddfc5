"""k_umap_layout and k_umap_dist (csrc/umap_kernels.hip) where tests/test_gpu_umap.py cannot see them: small-step runs
(learning_rate = 2^-10) of every k_umap_layout<G, C> instantiation against the fp64 reference, the firing schedule at large
t, the grid-stride tail of k_umap_dist, and run_umap as the composition of its parts.

The criterion is the project's: |Y - y64| <= 4 D32, D32 the distance between the reference's float32 and fp64 runs.  At a
small step every epoch's gradient is evaluated essentially at the start, nothing amplifies, and D32 is the storage rounding of
Y (one to a few f32 steps of a coordinate): the bound is then thousands of times tighter than the effect of a wrong negative
chain, a wrong schedule or a wrong coefficient, which tests/test_umap_host.py shows on the reference alone for every case
below."""
import numpy as np
import pytest

import umap_layout_cases as uc
import umap_reference as ref
from scrna_seq_qannealing_clustering_amd import umap

pytestmark = pytest.mark.gpu


def ulps(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert (a >= 0).all() and (b >= 0).all()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def check_small_step(case):
    g, c, neg, scale, seed, ab = case
    rowptr, col, w, Y0, y64, d32, moved = uc.reference(case)
    n = len(rowptr) - 1
    Y = umap.layout(rowptr, col, w, Y0, *uc.AB[ab], uc.T8, uc.LR, neg, seed)
    dev = float(np.abs(Y - y64).max())
    print("small step %s: D32 = %.3e, device = %.3e, moved = %.3e" % (uc.case_id(case), d32, dev, moved))
    assert Y.dtype == np.float32 and Y.shape == (n, c)
    assert d32 > 0.0 and moved >= 1000.0 * d32
    assert dev <= 4.0 * d32
    empty = np.diff(rowptr) == 0
    assert empty.any() and np.array_equal(Y[empty], Y0[empty])     # an empty row, bit for bit


@pytest.mark.parametrize("case", uc.INSTANCES, ids=uc.case_id)
def test_small_step_every_instantiation(case):
    """G in {16, 32, 64} (chosen through the mean row length, which uc.graph asserts) x c in {2, 3} x neg in {0, 1, 5, 16} x
    the starts normal * 4 and normal * 0.5 x seed 42 and a seed with a non-zero high word; every graph has an empty row, a row
    longer than G and a partly empty last wavefront.  Observed on an MI355X (per graph, c and start in the table of DESIGN.md
    section 5d): D32 8.69e-08 ... 2.53e-06, the device's error 8.69e-08 ... 2.53e-06 and at most 1.21 D32 (g32, c = 3, x 0.5,
    neg = 16: 2.11e-07 against 1.75e-07), equal to D32 in 69 of the 84 cases; largest move 0.010 ... 1.001, at least 3978 D32."""
    check_small_step(case)


@pytest.mark.parametrize("case", uc.THRESHOLDS, ids=uc.case_id)
def test_small_step_at_the_lane_group_thresholds(case):
    """Mean row lengths of exactly 16 and 32 (the narrower group: the selection is `> 16`, `> 32`) and of 16 + 1/n and
    32 + 1/n (the wider; an odd number of entries: one entry has no mirror, which the ABI allows).  The ABI does not report
    G: the mean is asserted and the result compared with the reference, which is all this test can see -- a wrong selection
    that computes the same sums in another order stays inside 4 D32.  Observed on an MI355X, D32 / device / largest move:
    mean16 1.75e-07 / 1.75e-07 / 0.152, mean16+ 1.51e-07 / 1.51e-07 / 0.130, mean32 1.70e-07 / 1.70e-07 / 0.244, mean32+
    1.67e-07 / 1.30e-07 / 0.226."""
    rowptr = uc.graph(case[0])[0]
    n = len(rowptr) - 1
    assert int(rowptr[-1]) == {"mean16": 16 * n, "mean16+": 16 * n + 1, "mean32": 32 * n, "mean32+": 32 * n + 1}[case[0]]
    check_small_step(case)


@pytest.mark.parametrize("case", uc.CURVES, ids=uc.case_id)
def test_small_step_other_curves(case):
    """find_ab_params(1.0, 0.3) (Seurat's default, b > 1) and a = b = 1 (both exp2_split trivial), one instantiation per c.
    Observed on an MI355X: the device's error equals D32 in all eight cases (1.04e-07 ... 1.99e-06),
    largest moves 0.019 ... 0.347."""
    check_small_step(case)


# ---- the schedule at large t ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [2, 3])
def test_small_step_500_epochs(c):
    """T = 500, n = 41 (mean row 14.2: 16 lanes), neg = 5, start x 0.5: floorf((t + 1) p) - floorf(t p) for t up to 499.
    Observed on an MI355X, D32 / device / largest move: c = 2 1.351e-06 / 1.401e-06 / 2.035, c = 3 1.282e-06 / 1.282e-06 /
    0.925."""
    rowptr, col, w = ref.degree_graph(41, 582, empty=(20,), hub=4, hub_deg=30, seed=41)
    Y0 = uc.start(41, c, 0.5)
    a, b = uc.AB["md0.1"]
    y64 = ref.layout(rowptr, col, w, Y0, a, b, uc.LR, 500, 5, 42, np.float64)
    y32 = ref.layout(rowptr, col, w, Y0, a, b, uc.LR, 500, 5, 42, np.float32)
    Y = umap.layout(rowptr, col, w, Y0, a, b, 500, uc.LR, 5, 42)
    d32, dev, moved = float(np.abs(y32 - y64).max()), float(np.abs(Y - y64).max()), float(np.abs(y64 - Y0).max())
    print("T = 500, c = %d: D32 = %.3e, device = %.3e, moved = %.3e" % (c, d32, dev, moved))
    assert d32 > 0.0 and moved >= 1000.0 * d32
    assert dev <= 4.0 * d32


def test_small_step_the_largest_epoch_count():
    """T = MI_UMAP_MAX_EPOCHS on ref.schedule_graph: eight vertices whose ratios p are 1, one f32 step below 1, float32(1/3),
    float32(2/3), float32(1/T) (fires once), 1/2, 1/4 and one step below float32(1/T) (never fires); neg = 1.  The edge that
    never fires can be removed without changing a bit of the result.  Observed on an MI355X: D32 9.769e-07, device 1.633e-06
    (1.67 D32), largest move 0.977."""
    T = umap.MAX_EPOCHS
    assert T == 10000
    rowptr, col, w, edges = ref.schedule_graph(T)
    fires = {e: ref.fire_counts(p, T) for e, p in edges.items()}
    assert fires == {(0, 1): T, (1, 2): T - 1, (2, 3): 3333, (3, 4): 6666, (4, 5): 1, (5, 6): T // 2, (0, 5): T // 4, (6, 7): 0}
    Y0 = uc.start(8, 2, 0.5)
    a, b = uc.AB["md0.1"]
    y64 = ref.layout(rowptr, col, w, Y0, a, b, uc.LR, T, 1, 42, np.float64)
    y32 = ref.layout(rowptr, col, w, Y0, a, b, uc.LR, T, 1, 42, np.float32)
    Y = umap.layout(rowptr, col, w, Y0, a, b, T, uc.LR, 1, 42)
    d32, dev, moved = float(np.abs(y32 - y64).max()), float(np.abs(Y - y64).max()), float(np.abs(y64 - Y0).max())
    print("T = %d: D32 = %.3e, device = %.3e, moved = %.3e" % (T, d32, dev, moved))
    assert d32 > 0.0 and moved >= 1000.0 * d32
    assert dev <= 4.0 * d32
    assert np.array_equal(Y[7], Y0[7])                             # its only edge never fires
    assert np.array_equal(Y, umap.layout(*ref.drop_edge(rowptr, col, w, 6, 7), Y0, a, b, T, uc.LR, 1, 42))


# ---- the grid-stride tail of k_umap_dist -----------------------------------------------------------------------------------

def test_knn_distances_past_the_launch_cap():
    """n k = 16 500 * 64 = 1 056 000 > 4096 * 256: the entries from 1 048 576 on (rows 16 384 ...) are written by the second
    trip of k_umap_dist's loop.  All entries against the specification's chain evaluated from the device's indices (2 f32
    steps, as check_graph of tests/test_gpu_umap.py); on 32 rows, 20 of them among the last 200 and 18 of those in the 116
    rows of the second trip (its first and its last row, the row before it and 16 drawn), the row's sorted distances
    against the 64 smallest exact fp64 distances (distances, not indices: a near-tie cannot fail it).  dim = 2: the chain
    differs from the exact distance by at most 1.5 steps (two rounded differences, two fmaf, sqrtf) plus the rounding of
    the exact value to f32."""
    n, k = 16500, 64
    assert n * k > 4096 * 256
    X = np.random.default_rng(16500).normal(size=(n, 2)).astype(np.float32)
    nn, dist = umap.knn(X, k, "euclidean")
    assert nn.shape == dist.shape == (n, k) and np.array_equal(nn[:, 0], np.arange(n)) and not dist[:, 0].any()
    assert ulps(dist, ref.distances(X, nn, "euclidean")).max() <= 2
    rng = np.random.default_rng(1)
    first = 4096 * 256 // k                                        # the first row that only the second trip writes
    assert n - 200 < first < n - 16
    rows = np.concatenate([rng.choice(n - 200, 12, replace=False), [n - 200, first - 1, first, n - 1],
                           first + 1 + rng.choice(n - first - 2, 16, replace=False)])
    assert len(set(rows.tolist())) == 32 and (rows >= n - 200).sum() == 20 and (rows * k >= 4096 * 256).sum() == 18
    X64 = X.astype(np.float64)
    exact = np.sqrt(((X64[rows, None, :] - X64[None, :, :]) ** 2).sum(axis=2))
    want = np.sort(exact, axis=1)[:, :k]
    assert ulps(np.sort(dist[rows], axis=1), want.astype(np.float32)).max() <= 2


# ---- run_umap is its parts ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("c", [2, 3])
def test_run_umap_is_fuzzy_graph_then_layout(c, metric):
    rng = np.random.default_rng(100 + c)
    X = rng.normal(size=(101, 5)).astype(np.float32)
    init = (rng.normal(size=(101, c)) * 3.0).astype(np.float32)
    r = umap.run_umap(X, n_neighbors=12, n_components=c, metric=metric, min_dist=0.1, n_epochs=20, learning_rate=0.25,
                      negative_sample_rate=3, init=init, seed=7)
    g = umap.fuzzy_graph(X, 12, metric)
    a, b = (float(np.float32(v)) for v in umap.find_ab_params(1.0, 0.1))
    Y = umap.layout(g.rowptr, g.col, g.weights, init, a, b, 20, 0.25, 3, 7)
    assert (r.a, r.b, r.n_epochs) == (a, b, 20)
    assert np.array_equal(r.rowptr, g.rowptr) and np.array_equal(r.col, g.col) and np.array_equal(r.weights, g.weights)
    assert np.array_equal(r.coords, Y)
    # ... and every one of those arguments reaches the kernel: another value is another result
    for kw in (dict(n_epochs=21), dict(learning_rate=0.5), dict(negative_sample_rate=4), dict(seed=8)):
        args = dict(n_epochs=20, learning_rate=0.25, negative_sample_rate=3, seed=7)
        args.update(kw)
        assert not np.array_equal(Y, umap.layout(g.rowptr, g.col, g.weights, init, a, b, **args)), kw
