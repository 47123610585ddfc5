"""Label agreement on the GPU (mi_label_agreement_u16, mi_sa_problem_label_agreement, csrc/agreement_kernels.hip)
against the numpy restatement of test_agreement_model.py: exact contingency tables and pair sums across the sizes where
the 64-cell chunks and the 16-label fragments change, with Ka != Kb, A != B and unused labels (a transposed or shifted
operand map shows up as a wrong table); WITHIN mode as the upper triangle of CROSS and groups as separate calls; no
int32 overflow at n = 100 000; the in-place pass over a padded-layout Potts anneal (holes skipped, the run untouched);
the sweep driver's stability and ari_to_previous.  numpy only (no sklearn on the GPU machine)."""
import ctypes as C
import math

import numpy as np
import pytest

from test_agreement_model import ref_ari, ref_contingency, ref_nmi, ref_pair_sum
from test_gpu_modularity import graph, problem
from scrna_seq_qannealing_clustering_amd import _lib, metrics, models
from scrna_seq_qannealing_clustering_amd.clustering import clustering_modularity_sweep
from scrna_seq_qannealing_clustering_amd.engine import Problem
from scrna_seq_qannealing_clustering_amd.sampler import default_potts_beta_range

pytestmark = pytest.mark.gpu

CROSS, WITHIN = 0, 1


def raw(A, B, Ka, Kb, mode=CROSS, groups=1, tables=True):
    """the C ABI with explicit K (unused labels included)"""
    A = np.ascontiguousarray(A, dtype=np.uint16)
    Ra, n = A.shape
    if mode == CROSS:
        B = np.ascontiguousarray(B, dtype=np.uint16)
        Rb = B.shape[0]
        P = Ra * Rb
    else:
        Rb, Rg = 0, Ra // groups
        P = groups * Rg * (Rg - 1) // 2
    ari, nmi, S = np.full(P, np.nan), np.full(P, np.nan), np.full(P, -1, dtype=np.int64)
    T = np.full((P, Ka, Kb), -1, dtype=np.int32) if tables else None
    u16p, f64p = C.POINTER(C.c_uint16), C.POINTER(C.c_double)
    ms = C.c_float(0)
    _lib.check(_lib.load().mi_label_agreement_u16(
        A.ctypes.data_as(u16p), Ra, B.ctypes.data_as(u16p) if mode == CROSS else None, Rb, n, Ka, Kb, mode, groups, 0,
        ari.ctypes.data_as(f64p), nmi.ctypes.data_as(f64p), S.ctypes.data_as(C.POINTER(C.c_int64)),
        T.ctypes.data_as(C.POINTER(C.c_int32)) if tables else None, C.byref(ms)))
    return ari, nmi, S, T


def near(rng, truth, K, p):
    out = truth.copy()
    flip = rng.random(truth.shape) < p
    out[flip] = rng.integers(0, K, int(flip.sum()))
    return out


# ---- 1. exact counts ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 2638])
@pytest.mark.parametrize("Ka,Kb", [(2, 16), (16, 17), (17, 64), (64, 2), (16, 16)])
def test_cross_exact(n, Ka, Kb):
    rng = np.random.default_rng(n * 131 + Ka * 7 + Kb)
    Ra, Rb = 5, 3
    # labels below K - 1 only in some rows: the top label stays unused there (its row / column of the table is 0)
    A = np.stack([rng.integers(0, max(Ka - (r % 2), 1), n) for r in range(Ra)])
    B = np.stack([near(rng, A[r % Ra] % Kb, max(Kb - (r % 2), 1), 0.3) for r in range(Rb)])
    ari, nmi, S, T = raw(A, B, Ka, Kb)
    for i in range(Ra):
        for j in range(Rb):
            p = i * Rb + j
            assert np.array_equal(T[p], ref_contingency(A[i], B[j], Ka, Kb)), (i, j)
            assert int(S[p]) == ref_pair_sum(A[i], B[j])
            assert abs(ari[p] - ref_ari(A[i], B[j])) <= 1e-12
            assert abs(nmi[p] - ref_nmi(A[i], B[j])) <= 1e-10


def test_public_functions_match_restatement():
    rng = np.random.default_rng(5)
    truth = rng.integers(0, 9, 2638)
    L = np.stack([near(rng, truth, 9, 0.1 * r) for r in range(6)])
    assert abs(metrics.adjusted_rand_index(L[1], truth) - ref_ari(L[1], truth)) <= 1e-12
    assert abs(metrics.normalized_mutual_info(L[2], truth) - ref_nmi(L[2], truth)) <= 1e-10
    many = metrics.adjusted_rand_index(L, truth)
    assert many.shape == (6,) and np.allclose(many, [ref_ari(x, truth) for x in L], rtol=0, atol=1e-12)
    assert np.array_equal(metrics.contingency(L[3], truth), ref_contingency(L[3], truth))
    # labels outside [0, 64) are compacted per labelling
    assert abs(metrics.adjusted_rand_index(L[1] * 1000 - 7, truth) - ref_ari(L[1], truth)) <= 1e-12
    ari, nmi = metrics.pairwise_agreement(L)
    assert ari.shape == (6, 6) and np.array_equal(ari, ari.T) and np.all(np.diag(ari) == 1.0)
    assert abs(ari[1, 4] - ref_ari(L[1], L[4])) <= 1e-12 and abs(nmi[4, 1] - ref_nmi(L[4], L[1])) <= 1e-10


# ---- 2. layout -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,R,G", [(16, 13, 1), (30, 12, 3), (64, 10, 2), (5, 9, 9)])
def test_within_is_upper_triangle_and_groups_are_separate_calls(K, R, G):
    rng = np.random.default_rng(K + R)
    truth = rng.integers(0, K, 700)
    A = np.stack([near(rng, truth, K, 0.05 * (r % 5)) for r in range(R)])
    Rg = R // G
    ari, nmi, S, _ = raw(A, None, K, K, WITHIN, G, tables=False)
    for g in range(G):
        blk = A[g * Rg:(g + 1) * Rg]
        ca, cn, cs, _ = raw(blk, blk, K, K, tables=False)
        iu = np.triu_indices(Rg, 1)
        flat = iu[0] * Rg + iu[1]
        P = Rg * (Rg - 1) // 2
        assert np.array_equal(S[g * P:(g + 1) * P], cs[flat])
        assert np.array_equal(ari[g * P:(g + 1) * P], ca[flat]) and np.array_equal(nmi[g * P:(g + 1) * P], cn[flat])
        sa, sn, ss, _ = raw(blk, None, K, K, WITHIN, 1, tables=False)
        assert np.array_equal(ss, S[g * P:(g + 1) * P]) and np.array_equal(sa, ari[g * P:(g + 1) * P])
        assert np.array_equal(sn, nmi[g * P:(g + 1) * P])
    for (r, s) in [(0, 1), (0, Rg - 1), (Rg - 2, Rg - 1)] if Rg > 1 else []:
        p = r * Rg - r * (r + 1) // 2 + (s - r - 1)
        assert int(S[p]) == ref_pair_sum(A[r], A[s]) and abs(ari[p] - ref_ari(A[r], A[s])) <= 1e-12


def test_many_labellings_tile_edges():
    """R not a multiple of any tile width, two groups: every pair against the restatement"""
    rng = np.random.default_rng(9)
    truth = rng.integers(0, 12, 300)
    A = np.stack([near(rng, truth, 12, 0.02 * (r % 11)) for r in range(38)])
    ari, nmi, S, _ = raw(A, None, 12, 12, WITHIN, 2, tables=False)
    p = 0
    for g in range(2):
        for r in range(19):
            for s in range(r + 1, 19):
                a, b = A[19 * g + r], A[19 * g + s]
                assert int(S[p]) == ref_pair_sum(a, b)
                assert abs(ari[p] - ref_ari(a, b)) <= 1e-12 and abs(nmi[p] - ref_nmi(a, b)) <= 1e-10
                p += 1


# ---- 3. no int32 overflow --------------------------------------------------------------------------------------------

def test_large_n_exact():
    n = 100000
    one = np.zeros(n, dtype=np.uint16)
    two = (np.arange(n) >= 30000).astype(np.uint16)
    A = np.stack([one, two])
    ari, nmi, S, T = raw(A, A, 2, 2)
    want_two = 30000 * 29999 // 2 + 70000 * 69999 // 2
    assert int(S[1]) == want_two and int(S[2]) == want_two and int(S[3]) == want_two
    assert int(S[0]) == n * (n - 1) // 2
    assert np.array_equal(T[1], [[30000, 70000], [0, 0]])
    assert ari[0] == 1.0 and nmi[0] == 1.0                     # both single-cluster
    assert ari[3] == 1.0 and abs(nmi[3] - 1.0) <= 1e-12        # identical
    assert ari[1] == 0.0 and nmi[1] == 0.0 and ari[2] == 0.0 and nmi[2] == 0.0
    single = np.stack([np.arange(n) % 64, np.arange(n) % 64]).astype(np.uint16)
    a2, n2, s2, _ = raw(single, None, 64, 64, WITHIN, 1, tables=False)
    assert a2[0] == 1.0 and int(s2[0]) == ref_pair_sum(single[0], single[1])


# ---- 4. padded layout, holes, continuation ---------------------------------------------------------------------------

def padded_run(continued, K=16):
    pm = models.build_modularity_potts(graph("s16"), 1.0, K)
    betas = models.make_beta_schedule(40, default_potts_beta_range(pm))
    with problem(pm, order="padded") as p:
        assert p.n_dev > pm.num_variables                       # holes present
        p.anneal(24, betas[:20], 7)
        agree = p.label_agreement() if continued else None
        p.anneal(24, betas[20:], 7, sweep_offset=20, continue_run=True)
        st, en, _ = p.fetch()
        agree2 = p.label_agreement(groups=3)
    return st, en, agree, agree2


def test_problem_label_agreement_matches_host_and_leaves_the_run():
    st, en, agree, agree2 = padded_run(True)
    st0, en0, _, _ = padded_run(False)
    assert np.array_equal(st, st0) and np.array_equal(en, en0)
    ari, nmi, S, _ = raw(st, None, 16, 16, WITHIN, 3, tables=False)
    assert agree2["ari"].shape == (3, 28)
    assert np.array_equal(agree2["pair_sum"].ravel(), S)
    assert np.allclose(agree2["ari"].ravel(), ari, rtol=0, atol=1e-13)
    assert np.allclose(agree2["nmi"].ravel(), nmi, rtol=0, atol=1e-13)
    assert agree["ari"].shape == (1, 24 * 23 // 2)


def test_problem_label_agreement_errors():
    pm = models.build_modularity_potts(graph("s16"), 1.0, 8)
    with problem(pm) as p:
        with pytest.raises(RuntimeError):
            p.label_agreement()
        with pytest.raises(_lib.MiSaError) as e:
            _lib.check(_lib.load().mi_sa_problem_label_agreement(p._h, 1, None, None, None, None))
        assert e.value.code == -6                                 # MI_ESTATE before any run
    Qs = np.eye(8, dtype=np.float32)
    with Problem.dense(Qs) as d:
        d.anneal(4, np.ones(3), 1)
        with pytest.raises(_lib.MiSaError) as e:
            _lib.check(_lib.load().mi_sa_problem_label_agreement(d._h, 1, None, None, None, None))
        assert e.value.code == -6


# ---- 5. the sweep driver ----------------------------------------------------------------------------------------------

def test_sweep_stability():
    G = graph("noisy_circles")
    kw = dict(num_reads=16, num_sweeps=60, seed=3)
    sets = clustering_modularity_sweep(G, [0.5, 1, 2], stability=True, sampler_kwargs=kw)
    prev = None
    for ss in sets:
        host = metrics.replica_stability(ss)
        assert ss.info["stability"] is not None and abs(ss.info["stability"] - host) <= 1e-12
        reads = np.repeat(ss.record["sample"], ss.record["num_occurrences"], axis=0)
        pairs = [(r, s) for r in range(len(reads)) for s in range(r + 1, len(reads))]
        want_nmi = math.fsum(ref_nmi(reads[r], reads[s]) for r, s in pairs) / len(pairs)
        assert abs(ss.info["stability_nmi"] - want_nmi) <= 1e-10
        best = np.asarray(ss.record["sample"][0])
        if prev is None:
            assert ss.info["ari_to_previous"] is None
        else:
            assert abs(ss.info["ari_to_previous"] - ref_ari(best, prev)) <= 1e-12
        prev = best
    plain = clustering_modularity_sweep(G, [0.5, 1, 2], sampler_kwargs=kw)
    for a, b in zip(plain, sets):
        assert set(b.info) - set(a.info) == {"stability", "stability_nmi", "ari_to_previous"}
        assert np.array_equal(a.record["sample"], b.record["sample"])
    one = clustering_modularity_sweep(G, [1.0], stability=True, sampler_kwargs=dict(kw, num_reads=1))
    assert one[0].info["stability"] is None and one[0].info["stability_nmi"] is None
