"""Merge moves on the Potts chain (chain 2e): a test-side restatement of the merge phase and of the
whole chain (chain 2d between merge phases, tests/test_modularity_model.py:chain2d), the energy change of a merge
against the model's fp64 energies, the fixed-point exponent and coefficient helpers, and the option checks the sampler
and the drivers make before any GPU work."""
import math

import numpy as np
import pytest

from conftest import GRAPH_NAMES, load_fixture
from oracle import sa_oracle as so
from test_modularity_model import bench_graph, chain2d
from scrna_seq_qannealing_clustering_amd import models


def merge_sums(lab, rowptr, col, vq, wq, K, hole):
    """Cluster sums W (integer weights), member counts N and the inter-cluster sums Bq[a][b] (a < b) of the fixed-point
    couplings ``vq``: each unordered edge once, from its entry (u, v) with l_u < l_v."""
    W = [0] * K
    N = [0] * K
    B = [[0] * K for _ in range(K)]
    for i in range(len(rowptr) - 1):
        if hole[i]:
            continue
        la = lab[i]
        W[la] += int(wq[i])
        N[la] += 1
        for e in range(rowptr[i], rowptr[i + 1]):
            lb = lab[col[e]]
            if la < lb:
                B[la][lb] += int(vq[e])
    return W, N, B


def merge_dE(B, W, a, b, f, cq):
    """dE of merging b into a: (double)Bq_ab 2^-f + cq (double)(W_a W_b), each product and the sum rounded once."""
    lo, hi = min(a, b), max(a, b)
    t1 = math.ldexp(float(B[lo][hi]), -f)
    t2 = cq * float(W[a] * W[b])
    return t1 + t2


def fixed_point(val, f):
    """vq = llrint(S_uv 2^f) (ties to even) of the fp32 couplings."""
    return np.rint(np.asarray(val, dtype=np.float32).astype(np.float64) * math.ldexp(1.0, f)).astype(np.int64)


def merge_phase(lab, rowptr, col, vq, wq, cq, K, P, s, gid, seed, T, f, hole, trace=None, replica=None):
    """One merge phase of chain 2e on the labels ``lab`` (a list, relabelled in place) before global sweep ``s`` at the
    fp32 temperature ``T``.  Returns the number of accepted merges.  ``trace``: a list that receives one
    ``(kind, replica, s, p, a, b, W_a W_b)`` per proposal, kind "accept", "empty" (the N == 0 skip) or "reject"."""
    W, N, B = merge_sums(lab, rowptr, col, vq, wq, K, hole)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    mp = list(range(K))
    acc = 0
    for p in range(P):
        w = so.philox4x32_10((p, s, gid, 4), key)
        a = w[0] % K
        b = (a + 1 + w[1] % (K - 1)) % K
        if N[a] == 0 or N[b] == 0:
            if trace is not None:
                trace.append(("empty", replica, s, p, a, b, W[a] * W[b]))
            continue
        dE = merge_dE(B, W, a, b, f, cq)
        thr = float(np.float32(so.neglog_u(w[2])) * np.float32(T))
        if trace is not None:
            trace.append(("accept" if dE < thr else "reject", replica, s, p, a, b, W[a] * W[b]))
        if not dE < thr:
            continue
        for c in range(K):
            if c == a or c == b:
                continue
            ia, ib = (min(a, c), max(a, c)), (min(b, c), max(b, c))
            B[ia[0]][ia[1]] += B[ib[0]][ib[1]]
            B[ib[0]][ib[1]] = 0
        B[min(a, b)][max(a, b)] = 0
        W[a] += W[b]
        W[b] = 0
        N[a] += N[b]
        N[b] = 0
        mp = [a if q == b else q for q in mp]
        acc += 1
    if acc:
        for i in range(len(lab)):
            if not hole[i]:
                lab[i] = mp[lab[i]]
    return acc


def chain2e(rowptr, col, val, wq, cw, cq, K, R, betas, seed, M, P, replica_offset=0, init=None, sweep_offset=0,
            absent=None, replicas=None, per_replica=None, trace=None):
    """Chain 2e: chain 2d with a merge phase of ``P`` proposals before every global sweep s = sweep_offset + local index
    with s > 0 and s % M == 0, at that sweep's temperature.  ``per_replica``: one constant beta per replica id (betas is
    then ignored for the temperatures, its length gives the sweep count).  ``trace``: see :func:`merge_phase` (replica =
    the id ``r``, without ``replica_offset``).  Returns (labels, accepted single-site moves, accepted merges)."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    n = len(rowptr) - 1
    hole = np.zeros(n, dtype=bool) if absent is None else np.asarray(absent, dtype=bool)
    f = models.merge_fixed_exponent(val)
    vq = fixed_point(val, f).tolist()
    rp, cl = rowptr.tolist(), col.tolist()
    ids = list(range(R)) if replicas is None else list(replicas)
    S = len(betas)
    out = np.zeros((len(ids), n), dtype=np.uint16)
    acc = merges = 0
    for k, r in enumerate(ids):
        gid = replica_offset + r
        if init is not None:
            lab = [int(x) for x in init[k]]
        else:
            lab = [0 if hole[i] else so.chain_word(seed, i, 0, gid, 1) % K for i in range(n)]
        rb = None if per_replica is None else np.full(S, per_replica[r])
        s0 = 0
        while s0 < S:
            s = sweep_offset + s0
            if s > 0 and s % M == 0:
                bt = rb[s0] if rb is not None else betas[s0]
                merges += merge_phase(lab, rp, cl, vq, wq, cq, K, P, s, gid, seed, np.float32(1.0 / bt), f, hole,
                                      trace=trace, replica=r)
            ln = min(S - s0, M - s % M)
            seg = (rb if rb is not None else np.asarray(betas))[s0:s0 + ln]
            lab2, a2, _ = chain2d(rowptr, col, val, wq, cw, K, R, seg, seed, replica_offset=replica_offset,
                                  init=np.asarray([lab]), sweep_offset=s, absent=hole, replicas=[r])
            lab = [int(x) for x in lab2[0]]
            acc += a2
            s0 += ln
        out[k] = lab
    return out, acc, merges


# ---- dE of a merge against the fp64 energies of the two labellings ----------------------------------------------------

def _check_dE(pm_chain, wq, cq, K, rng, trials=40):
    """``pm_chain``: the model as the chain sees it (fp32 couplings; quantised weights scaled back, if any)."""
    n = pm_chain.num_variables
    f = models.merge_fixed_exponent(pm_chain.val)
    vq = fixed_point(pm_chain.val, f)
    hole = np.zeros(n, dtype=bool)
    checked = 0
    for _ in range(trials):
        lab = rng.randint(0, K, size=n)
        W, N, B = merge_sums(lab.tolist(), pm_chain.rowptr.tolist(), pm_chain.col.tolist(), vq.tolist(), wq, K, hole)
        a, b = rng.choice(K, 2, replace=False)
        if N[a] == 0 or N[b] == 0:
            continue
        dE = merge_dE(B, W, a, b, f, cq)
        merged = np.where(lab == b, a, lab)
        e0, e1 = pm_chain.energies(np.stack([lab, merged]))
        scale = abs(math.ldexp(float(B[min(a, b)][max(a, b)]), -f)) + abs(cq * W[a] * W[b])
        assert dE == pytest.approx(e1 - e0, rel=1e-9, abs=1e-9 * scale)
        checked += 1
    assert checked > trials // 2


@pytest.mark.parametrize("name", GRAPH_NAMES)
def test_merge_dE_equals_energy_difference_dqm(name):
    pm = models.build_dqm_potts(load_fixture(name).graph(), 8, 0.005)
    c32 = float(np.float32(pm.c_pair))
    chain = models.PottsModel(pm.variables, pm.num_cases, pm.rowptr, pm.col,
                              pm.val.astype(np.float32).astype(np.float64), c32, pm.lin)
    _check_dE(chain, np.ones(pm.num_variables, dtype=np.int64), c32, 8, np.random.RandomState(4))


@pytest.mark.parametrize("name", ["bench", "noisy_circles", "blobs"])
def test_merge_dE_equals_energy_difference_modularity(name):
    G = bench_graph() if name == "bench" else load_fixture(name).graph()
    pm = models.build_modularity_potts(G, 1.0, 16)
    wq, cw, w64 = models.potts_node_weights(pm)
    e = pm.info["scale_exp"]
    cq = float(models.potts_merge_coefficients(pm)[0])
    # the chain's weights are wq 2^-e; its pair coefficient c
    chain = models.PottsModel(pm.variables, pm.num_cases, pm.rowptr, pm.col,
                              pm.val.astype(np.float32).astype(np.float64), pm.c_pair, pm.lin,
                              node_weight=np.ldexp(wq.astype(np.float64), -e))
    _check_dE(chain, wq.astype(np.int64), cq, 16, np.random.RandomState(5))


# ---- helpers ----------------------------------------------------------------------------------------------------------

def test_fixed_exponent():
    pm = models.build_modularity_potts(bench_graph(), 1.0, 16)
    v = np.abs(pm.val.astype(np.float32).astype(np.float64))
    total = float(np.add.accumulate(v)[-1])
    f = models.merge_fixed_exponent(pm.val)
    assert math.ldexp(total, f) <= 2.0 ** 62 < math.ldexp(total, f + 1)
    vq = fixed_point(pm.val, f)
    assert int(np.sum(np.abs(vq))) <= 2 ** 62 + len(vq)              # every Bq sum fits an int64
    assert models.merge_fixed_exponent(np.float32([2.0 ** 61, -(2.0 ** 61)])) == 0   # exactly 2^62 is allowed
    assert models.merge_fixed_exponent(np.float32([3.0])) == 60
    assert models.merge_fixed_exponent(np.zeros(0)) == 0
    assert models.merge_fixed_exponent(np.float32([1e-30])) == 161


def test_merge_coefficients():
    G = bench_graph()
    pm = models.build_modularity_potts(G, 0.8, 16)
    wq, cw, _ = models.potts_node_weights(pm)
    e = pm.info["scale_exp"]
    cq = models.potts_merge_coefficients(pm)
    assert cq.shape == (1,) and cq[0] == math.ldexp(pm.c_pair, -2 * e)
    # cq wq_u wq_v is the pair term c k_u k_v on the quantised degrees; cw_i = fp32(cq wq_i)
    assert np.array_equal(cw, (cq[0] * wq.astype(np.float64)).astype(np.float32))
    k = np.asarray(pm.node_weight)
    u, v = int(np.argmax(k)), int(np.argmin(k))
    assert cq[0] * float(wq[u]) * float(wq[v]) == pytest.approx(pm.c_pair * k[u] * k[v], rel=1e-5)
    sweep = models.build_modularity_sweep(G, [0.5, 1.0, 1.5], 16)
    cqs = models.potts_merge_coefficients(sweep)
    assert cqs.shape == (3,)
    assert np.array_equal(cqs, [models.potts_merge_coefficients(m)[0] for m in sweep])
    assert models.potts_merge_coefficients(models.build_dqm_potts(G, 8, 0.005)) is None


# ---- the restatement itself ---------------------------------------------------------------------------------------------

def _small_model():
    G = load_fixture("noisy_circles").graph()
    pm = models.build_modularity_potts(G, 1.0, 8)
    wq, cw, _ = models.potts_node_weights(pm)
    return pm, wq.astype(np.int64), cw, float(models.potts_merge_coefficients(pm)[0])


def test_chain2e_without_merge_points_is_chain2d():
    pm, wq, cw, cq = _small_model()
    v32 = pm.val.astype(np.float32)
    betas = models.make_beta_schedule(6, (0.5, 20.0))
    l2d, a2d, _ = chain2d(pm.rowptr, pm.col, v32, wq, cw, 8, 2, betas, 3)
    l2e, a2e, m2e = chain2e(pm.rowptr, pm.col, v32, wq, cw, cq, 8, 2, betas, 3, M=100, P=16)
    assert np.array_equal(l2d, l2e) and a2d == a2e and m2e == 0


def test_chain2e_merges_and_continues():
    """Cold merge phases accept merges; a run split at a merge boundary equals one run."""
    pm, wq, cw, cq = _small_model()
    v32 = pm.val.astype(np.float32)
    betas = models.make_beta_schedule(8, (5.0, 50.0))
    lab, acc, merges = chain2e(pm.rowptr, pm.col, v32, wq, cw, cq, 8, 2, betas, 11, M=4, P=16)
    assert merges > 0 and acc > 0
    first, a1, m1 = chain2e(pm.rowptr, pm.col, v32, wq, cw, cq, 8, 2, betas[:4], 11, M=4, P=16)
    rest, a2, m2 = chain2e(pm.rowptr, pm.col, v32, wq, cw, cq, 8, 2, betas[4:], 11, M=4, P=16, init=first,
                           sweep_offset=4)
    assert np.array_equal(rest, lab) and a1 + a2 == acc and m1 + m2 == merges


# ---- validation before any GPU work -----------------------------------------------------------------------------------

def test_sampler_validation_before_gpu(monkeypatch):
    from scrna_seq_qannealing_clustering_amd import engine, sampler as smod

    def no_gpu(*a, **k):
        raise AssertionError("GPU work started")

    monkeypatch.setattr(engine.Problem, "potts_csr", classmethod(lambda cls, *a, **k: no_gpu()))
    monkeypatch.setattr(smod._lib, "load", lambda: None)
    s = smod.MI355XSampler(device=0)
    G = load_fixture("blobs").graph()
    pm = models.build_modularity_potts(G, 1.0, 8)
    dqm = models.build_dqm_potts(G, 8, 0.005)
    cqm = models.build_cqm_potts(G, 4, 5)
    with pytest.raises(ValueError):
        s.sample_dqm(dqm, num_reads=4, num_sweeps=4, merge_interval=5, min_cluster_size=2)
    with pytest.raises(ValueError):
        s.sample_dqm(cqm, num_reads=4, num_sweeps=4, merge_interval=5)       # the model's own minimum size
    with pytest.raises(ValueError):
        s.sample_dqm(pm, num_reads=4, num_sweeps=4, merge_interval=-1)
    with pytest.raises(ValueError):
        s.sample_dqm(pm, num_reads=4, num_sweeps=4, merge_interval=5, merge_proposals=0)
    with pytest.raises(ValueError):
        s.sample_dqm_many([pm, models.build_modularity_potts(G, 0.5, 8)], num_reads=4, num_sweeps=4, merge_interval=-3)
    with pytest.raises(ValueError):
        s.sample_dqm_many([pm], num_reads=4, num_sweeps=4, merge_interval=5, min_cluster_size=2)
    assert "merge_interval" in smod.MI355XSampler.parameters and "merge_proposals" in smod.MI355XSampler.parameters


def test_driver_validation_before_gpu(monkeypatch):
    from scrna_seq_qannealing_clustering_amd import clustering, engine, sampler as smod

    monkeypatch.setattr(engine.Problem, "potts_csr",
                        classmethod(lambda cls, *a, **k: (_ for _ in ()).throw(AssertionError("GPU work started"))))
    monkeypatch.setattr(smod._lib, "load", lambda: None)
    G = load_fixture("blobs").graph()
    with pytest.raises(ValueError):
        clustering.clustering_modularity(G, 1.0, 8, merge_interval=-1, sampler_kwargs={"num_sweeps": 4, "num_reads": 4})
    with pytest.raises(ValueError):
        clustering.clustering_modularity_sweep(G, [0.5, 1.0], 8, merge_interval=-2,
                                               sampler_kwargs={"num_sweeps": 4, "num_reads": 4})
    with pytest.raises(ValueError):
        clustering.clustering_modularity(G, 1.0, 8, sampler_kwargs={"num_sweeps": 4, "num_reads": 4,
                                                                     "merge_interval": 5, "min_cluster_size": 2})
