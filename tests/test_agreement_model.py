"""Label agreement (ARI, NMI) without a GPU: the test-side restatement -- integer contingency by bincount, the
Hubert-Arabie closed form of ARI and the arithmetic NMI with sklearn's special cases -- pinned against sklearn; the
argument checks of metrics.py and of the C ABI, which run before any GPU call; replica_stability's expansion of
aggregated records (the device pass replaced by the restatement)."""
import ctypes as C
import math

import numpy as np
import pytest

from scrna_seq_qannealing_clustering_amd import _lib, metrics
from scrna_seq_qannealing_clustering_amd.sampleset import SampleSet


# ---- the restatement (the GPU tests import it) ----------------------------------------------------------------------

def ref_contingency(a, b, Ka=None, Kb=None):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    Ka = int(a.max()) + 1 if Ka is None else Ka
    Kb = int(b.max()) + 1 if Kb is None else Kb
    return np.bincount(a * Kb + b, minlength=Ka * Kb).reshape(Ka, Kb)


def comb2_sum(counts):
    """sum of C(c, 2), exact (Python integers)"""
    return sum(int(c) * (int(c) - 1) // 2 for c in np.asarray(counts).ravel())


def ref_pair_sum(a, b):
    return comb2_sum(ref_contingency(a, b))


def ref_ari(a, b):
    t = ref_contingency(a, b)
    n = len(a)
    S, A, B = comb2_sum(t), comb2_sum(t.sum(axis=1)), comb2_sum(t.sum(axis=0))
    if S == A and S == B:
        return 1.0
    c2 = n * (n - 1) / 2.0
    p = float(A) * float(B) / c2
    den = 0.5 * (A + B) - p
    return 1.0 if den == 0 else (S - p) / den


def _entropy(counts, n):
    c = np.asarray(counts, dtype=np.float64)
    c = c[c > 0]
    return float(-np.sum(c / n * np.log(c / n)))


def ref_nmi(a, b):
    t = ref_contingency(a, b)
    n = len(a)
    ra, rb = t.sum(axis=1), t.sum(axis=0)
    ka, kb = int((ra > 0).sum()), int((rb > 0).sum())
    if ka == 1 and kb == 1:
        return 1.0
    if ka == 1 or kb == 1:
        return 0.0
    i, j = np.nonzero(t)
    nij = t[i, j].astype(np.float64)
    mi = float(np.sum(nij / n * (np.log(nij) + math.log(n) - np.log(ra[i].astype(np.float64)) - np.log(rb[j].astype(np.float64)))))
    mi = max(mi, 0.0)
    if mi == 0.0:
        return 0.0
    return mi / (0.5 * (_entropy(ra, n) + _entropy(rb, n)))


def agreement_cases(rng):
    """(name, a, b): random labellings near a planted truth, and the degenerate ones"""
    out = []
    for n, K in ((2638, 16), (500, 9), (65, 3), (2, 2)):
        truth = rng.integers(0, K, n)
        noisy = truth.copy()
        flip = rng.random(n) < 0.2
        noisy[flip] = rng.integers(0, K, int(flip.sum()))
        out.append(("random_%d_%d" % (n, K), truth, noisy))
        out.append(("independent_%d_%d" % (n, K), truth, rng.integers(0, K + 3, n)))
    a = rng.integers(0, 7, 300)
    perm = rng.permutation(7)
    out += [("identical", a, a.copy()), ("permuted", a, perm[a]), ("single_both", np.zeros(50, int), np.zeros(50, int)),
            ("single_one_side", np.zeros(50, int), rng.integers(0, 4, 50)),
            ("single_other_side", rng.integers(0, 4, 50), np.zeros(50, int)),
            ("singletons_both", np.arange(40), np.arange(40)[::-1].copy()),
            ("singletons_vs_blocks", np.arange(40), np.arange(40) // 8), ("one_cell", np.zeros(1, int), np.zeros(1, int))]
    return out


CASES = agreement_cases(np.random.default_rng(11))


@pytest.mark.parametrize("name,a,b", CASES, ids=[c[0] for c in CASES])
def test_restatement_matches_sklearn(name, a, b):
    skm = pytest.importorskip("sklearn.metrics")
    assert abs(ref_ari(a, b) - skm.adjusted_rand_score(a, b)) <= 1e-12
    assert abs(ref_nmi(a, b) - skm.normalized_mutual_info_score(a, b)) <= 1e-12
    assert ref_pair_sum(a, b) == comb2_sum(skm.cluster.contingency_matrix(a, b))


def test_restatement_closed_forms_hold_beyond_int32():
    n = 100000
    a, b = np.zeros(n, int), (np.arange(n) >= 30000).astype(int)
    assert ref_pair_sum(a, b) == 30000 * 29999 // 2 + 70000 * 69999 // 2 > 2 ** 31
    assert ref_ari(a, b) == 0.0 and ref_nmi(a, b) == 0.0
    assert ref_ari(a, a) == 1.0 and ref_nmi(a, a) == 1.0 and ref_ari(b, b) == 1.0


# ---- argument checks before any GPU call ---------------------------------------------------------------------------

@pytest.fixture
def no_gpu(monkeypatch):
    """fails the test if the native pass is reached"""
    def boom(*a, **k):
        raise AssertionError("the native pass was called")
    monkeypatch.setattr(metrics, "_lib", type("L", (), {"load": staticmethod(boom), "check": staticmethod(boom)}))


def test_metrics_validation_before_gpu(no_gpu):
    with pytest.raises(ValueError, match="distinct labels"):
        metrics.adjusted_rand_index(np.arange(65), np.zeros(65, int))
    with pytest.raises(ValueError, match="different numbers of cells"):
        metrics.label_agreement(np.zeros((2, 5), int), np.zeros((1, 6), int))
    with pytest.raises(ValueError, match="equal groups"):
        metrics.pairwise_agreement(np.zeros((5, 4), int), groups=2)
    with pytest.raises(ValueError, match="at least one"):
        metrics.label_agreement(np.zeros((0, 4), int))
    with pytest.raises(ValueError, match="shape"):
        metrics.normalized_mutual_info(np.zeros(4, int), np.zeros((2, 4), int))
    with pytest.raises(ValueError, match="pairs across"):
        metrics.label_agreement(np.zeros((4, 4), int), tables=True)


def test_compaction_of_labels_outside_range():
    L, K = metrics._labellings(np.array([[100, -5, 100, 7], [0, 1, 2, 3]]), "A")
    assert K == 4
    assert L.tolist() == [[2, 0, 2, 1], [0, 1, 2, 3]]
    L, K = metrics._labellings(np.array(["x", "y", "x"]), "A")
    assert L.tolist() == [[0, 1, 0]] and K == 2


def _abi(A, Ra, B, Rb, n, Ka, Kb, mode, groups, tables=None):
    """``tables``: an out_tables pointer for a call that is refused before anything is written (None: NULL)"""
    u16p = C.POINTER(C.c_uint16)
    A = np.ascontiguousarray(A, dtype=np.uint16)
    Bp = np.ascontiguousarray(B, dtype=np.uint16).ctypes.data_as(u16p) if B is not None else None
    return _lib.load().mi_label_agreement_u16(A.ctypes.data_as(u16p), Ra, Bp, Rb, n, Ka, Kb, mode, groups, 0,
                                              None, None, None, tables, None)


# never dereferenced: mi_label_agreement_u16 refuses the call on its shape, before it reads a label or looks for a device
DUMMY_TABLES = C.cast(C.c_void_p(8), C.POINTER(C.c_int32))


REFUSAL_CODE = {"exceed": -5}     # MI_EUNSUPPORTED; every other message comes with MI_EINVAL (-1)


@pytest.mark.parametrize("args,msg", [
    ((np.zeros((2, 4)), 2, np.zeros((2, 4)), 2, 0, 2, 2, 0, 1), "n must be"),
    ((np.zeros((2, 4)), 2, np.zeros((2, 4)), 2, 4, 65, 2, 0, 1), "Ka must be"),
    ((np.zeros((2, 4)), 2, np.zeros((2, 4)), 2, 4, 2, 0, 0, 1), "Kb must be"),
    ((np.full((2, 4), 3), 2, np.zeros((2, 4)), 2, 4, 3, 2, 0, 1), "outside"),
    ((np.zeros((2, 4)), 2, np.full((2, 4), 2), 2, 4, 3, 2, 0, 1), "outside"),
    ((np.zeros((2, 4)), 2, None, 0, 4, 2, 2, 0, 1), "needs B"),
    ((np.zeros((2, 4)), 2, np.zeros((2, 4)), 2, 4, 2, 2, 1, 1), "B = NULL"),
    ((np.zeros((6, 4)), 6, None, 0, 4, 2, 2, 1, 4), "multiple of groups"),
    ((np.zeros((2, 4)), 2, np.zeros((2, 4)), 2, 4, 2, 2, 0, 2), "groups = 1"),
    ((np.zeros((2, 4)), 2, np.zeros((2, 4)), 2, 4, 2, 2, 7, 1), "mode must be"),
    ((np.zeros((2, 4)), 0, np.zeros((2, 4)), 2, 4, 2, 2, 0, 1), "Ra must be"),
    # above MI_AGREE_MAX_LABELLINGS: refused on the shape, before the labels (here 8 of them) are read
    ((np.zeros((2, 4)), 65537, np.zeros((2, 4)), 2, 4, 2, 2, 0, 1), "Ra must be"),
    ((np.zeros((2, 4)), 2, np.zeros((2, 4)), 65537, 4, 2, 2, 0, 1), "Rb must be"),
    # 300 x 300 tables of 64 x 64 = 3.7e8 entries > MI_AGREE_MAX_TABLE_ENTRIES = 2^28: MI_EUNSUPPORTED, with tables only
    ((np.zeros((300, 4)), 300, np.zeros((300, 4)), 300, 4, 64, 64, 0, 1, DUMMY_TABLES), "exceed"),
])
def test_abi_validation_before_device(args, msg):
    assert _abi(*args) == REFUSAL_CODE.get(msg, -1)              # MI_EINVAL / MI_EUNSUPPORTED, not MI_ENODEV: no device is looked for
    assert msg in _lib.load().mi_last_error().decode()


# ---- replica_stability over reads ----------------------------------------------------------------------------------

def fake_label_agreement(A, B=None, groups=1, device=0, tables=False):
    L, _ = metrics._labellings(A, "A")
    assert B is None and groups == 1
    pairs = [(r, s) for r in range(L.shape[0]) for s in range(r + 1, L.shape[0])]
    return {"ari": np.array([ref_ari(L[r], L[s]) for r, s in pairs]),
            "nmi": np.array([ref_nmi(L[r], L[s]) for r, s in pairs]), "pair_sum": None, "tables": None, "kernel_ms": 0.0}


def test_replica_stability_expands_aggregated_records(monkeypatch):
    monkeypatch.setattr(metrics, "label_agreement", fake_label_agreement)
    rng = np.random.default_rng(3)
    base = rng.integers(0, 4, (3, 30))
    reads = base[[0, 0, 1, 2, 2, 2, 1]]                           # 7 reads, 3 distinct
    ss = SampleSet(reads, rng.random(3)[[0, 0, 1, 2, 2, 2, 1]], list(range(30)), "DISCRETE")
    assert len(ss.record) == 3 and int(ss.record["num_occurrences"].sum()) == 7
    pairs = [(r, s) for r in range(7) for s in range(r + 1, 7)]
    want = math.fsum(ref_ari(reads[r], reads[s]) for r, s in pairs) / len(pairs)
    assert abs(metrics.replica_stability(ss) - want) <= 1e-12
    one = SampleSet(reads[:1], np.zeros(1), list(range(30)), "DISCRETE")
    assert metrics.replica_stability(one) is None
