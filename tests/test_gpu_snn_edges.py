"""GPU SNN construction (csrc/snn_kernels.hip) against oracle/snn_oracle.c at the edges of its kernels: every k_knn
template instance with short and ragged tiles, tie-ridden lattices, subnormal and near-overflow squared distances, the
1024-element passes of the scan, SNN rows around the bitonic sort's powers of two and at the row cap, the hub refusal,
the sequential trim kernel, pruning exactly at a weight, and run-to-run repeatability.  Everything is integer output:
nn, rowptr, col, shared (and code) bit for bit, no tolerance anywhere.  The inputs come from tests/snn_cases.py and
tests/test_snn_host.py establishes, with the oracle alone, that they are what the cases below take them to be."""
import numpy as np
import pytest

import snn_cases as sc
from oracle import snn_oracle as sn
from scrna_seq_qannealing_clustering_amd import _lib, snn

pytestmark = pytest.mark.gpu

EUNSUPPORTED = -5


def assert_equals_oracle(g, want, what=""):
    """g: SnnGraph; want: the oracle's (nn, rowptr, col, shared[, code])"""
    names = ("nn", "rowptr", "col", "shared", "code")
    for name, w in zip(names, want):
        assert np.array_equal(getattr(g, name), w), "%s differs from the oracle %s" % (name, what)


def assert_same_graph(a, b, what=""):
    for name in ("nn", "rowptr", "col", "shared", "code"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), "%s differs %s" % (name, what)


def check_plain(X, k, prune=0.0, ord_=None, what=""):
    g = snn.build_snn(X, k, prune, ord_)
    assert_equals_oracle(g, sn.snn_graph(X, k, prune, ord_), what)
    return g


# ---- 1. the k_knn dispatch matrix -----------------------------------------------------------------------------------------
# DP = 16 | 32 | 64 switches at dim 16|17 and 32|33; KM = 8 | 16 | 32 | 64 at k - 1 = 8|9, 16|17, 32|33; n < 64 is a short
# single tile, n % 4 != 0 leaves a ragged last group of four, n = 65 .. 67 and 129 a last tile of one to three candidates.

DISPATCH_DIMS = (1, 4, 5, 16, 17, 32, 33, 63, 64)
DISPATCH_KS = (2, 9, 10, 17, 18, 33, 34, 64)


@pytest.mark.parametrize("n", [2, 3, 5, 63, 64, 65, 66, 67, 129, 257])
def test_knn_dispatch_matrix(n):
    ks = [k for k in DISPATCH_KS if k <= n]
    if n <= 64 and n not in ks:
        ks.append(n)                                              # k == n: every other point is a neighbour
    cases = 0
    for dim in DISPATCH_DIMS:
        X = sc.cloud(n, dim, seed=1000 * n + dim)
        for k in ks:
            ord_ = None if cases % 2 == 0 else 4
            check_plain(X, k, 0.0, ord_, "(n=%d dim=%d k=%d ord=%s)" % (n, dim, k, ord_))
            cases += 1
    assert cases == len(DISPATCH_DIMS) * len(ks) and cases >= len(DISPATCH_DIMS)


# ---- 2. ties ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,dim,levels", sc.LATTICES)
def test_lattice_ties_resolve_by_index(n, dim, levels):
    X = sc.lattice(n, dim, levels)
    for k in sc.LATTICE_KS:
        for ord_ in (None, 6):
            check_plain(X, k, 0.0, ord_, "(lattice n=%d dim=%d k=%d ord=%s)" % (n, dim, k, ord_))


def test_duplicates_across_the_tile_boundary():
    X = sc.duplicates_across_tile()
    for k in (9, 18):
        g = check_plain(X, k, 0.0, None, "(duplicates, k=%d)" % k)
        first = [j for j in range(56, 72) if j != 60][:k - 1]   # the 15 twins of point 60, lowest index first
        assert g.nn[60, 1:1 + len(first)].tolist() == first


# ---- 3. magnitudes ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["subnormal", "near_overflow", "offset_1e6"])
def test_magnitudes(name):
    """The oracle is IEEE fp32 with subnormals: a kernel that flushed them, or evaluated the chain in another order or
    precision, would order these neighbours differently."""
    X, k = sc.magnitude_cases()[name]
    for ord_ in (None, 4):
        check_plain(X, k, 0.0, ord_, "(%s, ord=%s)" % (name, ord_))


# ---- 4. the 1024-element passes of k_scan_exclusive -------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1023, 1024, 1025, 2048, 2049])
def test_scan_passes(n):
    check_plain(sc.cloud(n, 8, seed=n), 5, 0.0, 15, "(n=%d)" % n)


# ---- 5. row sizes of k_snn_rows, the row cap and the hub refusal ------------------------------------------------------------

@pytest.mark.parametrize("n", [257, 258, 513, 514, 1025])
def test_star_rows_around_powers_of_two(n):
    """Rows of n - 1 = 256 | 257, 512 | 513, 1024 candidates: several emit passes per thread, bitonic padding to 256, 512,
    1024.  With ord = 15 every column of the trim depends on every smaller one: the parallel trim runs serialised and may
    fall back to the sequential kernel; the result is the oracle's on either path."""
    X = sc.star(n)
    g = check_plain(X, sc.STAR_K, 0.0, None, "(star %d, untrimmed)" % n)
    assert np.array_equal(np.diff(g.rowptr), np.full(n, n - 1))
    check_plain(X, sc.STAR_K, 0.0, 15, "(star %d, ord=15)" % n)


def test_rows_at_the_cap_are_accepted_and_one_more_is_refused():
    n = sc.ROW_CAP + 1
    g = check_plain(sc.star(n), sc.STAR_K, 0.0, None, "(star %d)" % n)
    assert np.array_equal(np.diff(g.rowptr), np.full(n, sc.ROW_CAP))
    with pytest.raises(_lib.MiSaError) as ei:
        snn.build_snn(sc.star(n + 1), sc.STAR_K, 0.0, None)
    assert ei.value.code == EUNSUPPORTED and "hub" in ei.value.message
    check_plain(sc.cloud(300, 15, seed=9), 5, 0.0, 15, "(after the hub refusal)")       # the library is still usable


# ---- 6. the sequential trim kernel ----------------------------------------------------------------------------------------

def _forced_sequential_cases():
    return [
        ("plain", sc.cloud(777, 15, seed=7 * 777 + 16), 16, dict(prune=1 / 15, ord=16)),
        ("star", sc.star(513), sc.STAR_K, dict(ord=15)),
        ("rounded", sc.cloud(1200, 10, seed=7 * 1200 + 30, clusters=5), 30, dict(ord=12, round_digits=2, negative_below=0.05)),
        ("mutual_ord2", sc.cloud(300, 15, seed=5 * 300 + 5), 5, dict(ord=15, enhance="mutual", ord2=9)),
        ("sum_unsymmetric_ord2", sc.cloud(900, 30, seed=5 * 900 + 10), 10, dict(ord=12, enhance="sum", symmetric=False, ord2=7)),
    ]


@pytest.mark.parametrize("case", range(5), ids=[c[0] for c in _forced_sequential_cases()])
def test_forced_sequential_trim(case, monkeypatch):
    name, X, k, kw = _forced_sequential_cases()[case]
    prune, ord_ = kw.get("prune", 0.0), kw["ord"]
    if "round_digits" in kw:
        want = sn.snn_graph_rounded(X, k, prune, ord_, kw["round_digits"], kw["negative_below"])
    elif "enhance" in kw:
        want = sn.snn_graph_variant(X, k, prune, ord_, kw.get("symmetric", True), kw["enhance"], 2.0, kw["ord2"])
    else:
        want = sn.snn_graph(X, k, prune, ord_)
    assert int(np.diff(sn.snn_rows(want[0], prune)[0]).max()) > ord_          # some column exceeds the cap: the trim deletes
    extra = {key: v for key, v in kw.items() if key not in ("prune", "ord")}
    monkeypatch.delenv("MI_SNN_TRIM_SEQUENTIAL", raising=False)
    default = snn.build_snn(X, k, prune, ord_, **extra)
    monkeypatch.setenv("MI_SNN_TRIM_SEQUENTIAL", "1")              # read by the library at every build
    forced = snn.build_snn(X, k, prune, ord_, **extra)
    assert_equals_oracle(forced, want, "(%s, sequential trim)" % name)
    assert_equals_oracle(default, want, "(%s, default trim)" % name)
    assert_same_graph(forced, default, "between the sequential and the default trim (%s)" % name)


# ---- 7. prune exactly at a weight ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", [1, 3, 7])
def test_prune_at_equality(s):
    """s / (2k - s) >= prune keeps an entry: at prune equal to that weight, computed as the kernel computes it, the entries
    with s shared neighbours stay; one ulp above they are gone."""
    k = 8
    X = sc.cloud(600, 3, seed=31)
    prune = float(s) / (2.0 * k - float(s))
    at = check_plain(X, k, prune, None, "(prune at s=%d)" % s)
    above = check_plain(X, k, float(np.nextafter(prune, 1.0)), None, "(prune one ulp above s=%d)" % s)
    assert (at.shared == s).any() and at.shared.min() == s
    assert not (above.shared == s).any() and above.shared.min() == s + 1


# ---- 8. repeatability -------------------------------------------------------------------------------------------------------

def test_two_builds_are_identical():
    """The reverse-neighbour lists are filled in the order atomics arrive; the row sort must hide that."""
    for X, k, ord_ in ((sc.star(514), sc.STAR_K, 15), (sc.star(514), sc.STAR_K, None), (sc.lattice(300, 3, 3), 17, 6)):
        a, b = snn.build_snn(X, k, 0.0, ord_), snn.build_snn(X, k, 0.0, ord_)
        assert_same_graph(a, b, "between two builds")
