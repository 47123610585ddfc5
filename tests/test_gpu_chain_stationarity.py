"""Every kernel family samples exp(-beta E): chi-square against fp64 enumeration, the oracle not in the loop.

Same models and the same fixed pass rule as tests/test_chain_stationarity.py (tests/chain_stats.py: p >= 1e-6,
|z| <= 5, pooled bin <= 5 % of the mass), through ``engine.Problem`` with the kernel forced by the options the parity
tests use and ``kernel_name()`` asserted in every case.  Each case also counts the accepted moves of ONE further sweep
(a continued call) against their exact expectation under stationarity (within 5 standard errors): a kernel whose
counters and states disagree fails there.

2^18 replicas go into one ``anneal`` call wherever the kernel takes them -- a launch shape no parity test reaches (the
largest R there is 4096-8192).  Which cases do not, and why:

* the few-replica forms (K2w / K2s, K2 with ``k2_waves``, K2p and K3f beside a threshold wavefront) are chosen by the read
  count (up to 1024; K2p ``tw`` up to 16 replicas per CU): 2^15 samples accumulated over calls with distinct
  ``replica_offset``, on models of 64-81 states so that the bins still expect 5;
* K1x / K1g exist for n > 4096 only: the 6-variable model is embedded in 4097 variables (the others uncoupled with a
  linear term of 64: beta * 64 > 23 ln 2, the largest -ln u of the chain, so once 0 they never move; asserted), 2^12
  replicas in one call -- 2^18 would be 1 GiB of states and 4e13 proposals for a 64-state model;
* K2 keeps a 16-bit state cell per variable on every model up to 4608 variables; its byte / bit state forms, the library's
  choice beyond, run here under ``MI_K2_STATE`` (read when the model is created; the cases named "byte" / "bit"):
  ``k_anneal_csr_rank1<16, 1>`` and ``<16, 0>`` at 2^18 replicas, one of them with the weighted slot, and both beside their
  threshold wavefront (``<16, 1, tw>``, ``<16, 0, tw>``) in calls of 1024 replicas.  D = 32 / 64 / the runtime width of K2
  stay pinned by oracle parity alone (tests/test_gpu_k2_state_forms.py): a row of 17 neighbours needs n = 18, and 2^18
  states cannot each expect 5 of 2^18 samples;
* K3 / K3f with 32 adjacency entries need a variable with 17 neighbours, so n = 18: with K = 2 the 2^18 labelings can
  be enumerated but cannot each expect 5 samples, so 12 leaves are tied to the hub and move with it as one variable
  (chain_stats.hub_model says why the block's label is still exactly Boltzmann); K3f's 16-label form at that width
  (K >= 9, n >= 18) is beyond enumeration and not covered.

What ``kernel_name()`` does not show: K2's workgroup shape (``k2_waves``, few reads) is not part of its name and the
library exposes it nowhere else, so for "K2 few reads" and "K2 three waves" the assertion shows that K2 was taken, not
in which shape; and the single counted sweep of the scheduler case (variant 4) is too short to be chunked, so it runs on
K1w alone -- the 50 judged sweeps before it ran on both kernels, as the asserted name shows.

The GPU is shared: every case is one or a few launches on register-sized models, nothing loops on a failure.
Measured on an MI355X: 8 s for the file (65 cases), 0.01 - 0.23 s per case (``pytest -s`` prints kernel, R per call, p, z, acceptance deviation and
wall time per case; DESIGN.md section 6, "what pins the chain").
"""
import time

import numpy as np
import pytest

import chain_stats as cs
from scrna_seq_qannealing_clustering_amd import tempering
from scrna_seq_qannealing_clustering_amd.engine import Problem
from chain_stats import PT_CHAINS, PT_LADDER, csr_model, hub_model, judge_rungs, potts_model

pytestmark = pytest.mark.gpu

R = 1 << 18
R_FEW = 1 << 15
S = 50


def sample(p, beta, seed, r_call=R, total=R, init=None, options=(), betas=None):
    """``total`` replicas in calls of ``r_call`` (distinct ``replica_offset``): S sweeps at ``beta`` from the tag-1 (or
    given) initial state, then ONE continued sweep whose accepted moves are counted.  Returns states, energies, that
    count, the kernel name (the same in every call) and the wall time."""
    for k, v in options:
        p.set_option(k, v)
    t0 = time.perf_counter()
    sts, ens, acc, name = [], [], 0, None
    burn = np.full(S, beta) if betas is None else np.repeat(np.asarray(betas, dtype=np.float64)[:, None], S, axis=1)
    for ro in range(0, total, r_call):
        p.anneal(r_call, burn, seed, replica_offset=ro, initial_states=None if init is None else init[:r_call])
        st, en, _ = p.fetch()
        this = p.kernel_name()
        assert name in (None, this), (name, this)
        name = this
        p.anneal(r_call, burn[..., :1], seed, replica_offset=ro, sweep_offset=S, continue_run=True)
        assert all(part in name for part in p.kernel_name().split(" + ")), (p.kernel_name(), name)
        acc += p.fetch(states=False)[2]["accepted"]
        sts.append(st)
        ens.append(en)
    return np.concatenate(sts), np.concatenate(ens), acc, name, time.perf_counter() - t0


def device_order(p, n):
    """The order in which the device proposes the caller's variables within a sweep."""
    return list(range(n)) if p._inv is None else [int(i) for i in np.argsort(p._inv)]


def report(name, kernel, r_call, wall):
    print("    %-44s %s, R per call %d, %.2f s" % (name, kernel, r_call, wall))


# ---- dense -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,unit_rows,kernel", [
    (1, 0, "k_anneal_dense<4>"), (2, 2, "k_anneal_dense_wg<4,2>"), (2, 4, "k_anneal_dense_wg<4,4>"),
    (3, 0, "k_anneal_dense_mfma<4>"), (4, 0, "k_anneal_dense_mfma<4> + k_anneal_dense_wg<4,4>")])
@pytest.mark.parametrize("n,beta", [(8, 1.0), (1, 2.0), (5, 0.3)])
def test_dense_kernels(variant, unit_rows, kernel, n, beta):
    Qs = cs.random_dense(n, 100 + n)
    X, E = cs.enumerate_binary(Qs=Qs)
    pi = cs.reference(E, beta, R)
    with Problem.dense(Qs) as p:
        st, en, acc, name, wall = sample(p, beta, 7, options=(("variant", variant), ("unit_rows", unit_rows)))
    report("dense n=%d variant %d/%d" % (n, variant, unit_rows), name, R, wall)
    assert name == kernel, name
    cs.judge("2a %s n=%d beta=%g" % (name, n, beta), cs.binary_index(st), en, E, pi, 1e-4, acc,
             cs.accept_moments_binary(E, n, beta, pi))


@pytest.mark.parametrize("mode,chain,kernel", [
    (2, 0, "k_anneal_dense_xl<2>"),
    (1, 2, "k_xg_chain + k_xg_panel (K1g, 65 blocks of 64 rows in groups of 8)"),
    (1, 1, "k_xg_diag + k_xg_panel (K1g, 65 blocks of 64 rows in groups of 8)")])
def test_dense_large_model_kernels_on_an_embedded_model(mode, chain, kernel):
    n, n_total, beta, Rx = 6, 4097, 0.6, 1 << 12
    Qs = cs.random_dense(n, 106)
    X, E = cs.enumerate_binary(Qs=Qs)
    pi = cs.reference(E, beta, Rx)
    assert beta * 64.0 > 23 * np.log(2.0)
    with Problem.dense(cs.embed_dense(Qs, n_total)) as p:
        st, en, acc, name, wall = sample(p, beta, 7, r_call=Rx, total=Rx, options=(("xl_batched", mode), ("xl_chain", chain),
                                                                             ("xl_cold_permille", 0)))     # (K1g never hands over to K1x)
    report("dense embedded in %d, xl_batched %d" % (n_total, mode), name, Rx, wall)
    assert name == kernel, name
    assert not st[:, n:].any()
    cs.judge("2a %s n=6 in 4097 beta=%g" % (kernel.split(" (")[0], beta), cs.binary_index(st[:, :n]), en, E, pi, 1e-4, acc,
             cs.accept_moments_binary(E, n, beta, pi))


# ---- structured binary ---------------------------------------------------------------------------------------------------
def csr6():
    """The 64-state structured model of the few-replica cases."""
    rp, col, val = cs.random_graph(6, 26)
    return rp, col, val, (np.random.RandomState(27).randn(6) * 0.5).astype(np.float32), 0.11


def force_k2_state(monkeypatch, case):
    """MI_K2_STATE (read when the model is created) for a case named "... byte ..." / "... bit ...", unset for the others."""
    monkeypatch.delenv("MI_K2_STATE", raising=False)
    for state in ("byte", "bit"):
        if state in case.split():
            monkeypatch.setenv("MI_K2_STATE", state)


@pytest.mark.parametrize("case,kind,order,options,beta,kernel", [
    ("K2", "pair", None, (("k2_pair", 0),), 0.5, "k_anneal_csr_rank1<16, 2>"),
    ("K2", "pair", None, (("k2_pair", 0),), 2.0, "k_anneal_csr_rank1<16, 2>"),
    ("K2 c=0", "c0", None, (("k2_pair", 0),), 2.0, "k_anneal_csr_rank1<16, 2>"),
    ("K2p", "pair", "padded", (("k2_pair", 1), ("k2_tw", 2)), 0.5, "k_anneal_csr_rank1_pair<16>"),
    ("K2p", "pair", "padded", (("k2_pair", 1), ("k2_tw", 2)), 2.0, "k_anneal_csr_rank1_pair<16>"),
    ("K2 padded", "pair", "padded", (("k2_pair", 2), ("k2_split", 2)), 2.0, "k_anneal_csr_rank1<16, 2>"),
    ("slots", "pair", "slots", (), 0.5, "k_anneal_csr_rank1<16, 2>"),
    ("K2p tw weighted", "weighted", "padded", (), 0.5, "k_anneal_csr_rank1_pair<16, tw>"),
    ("K2p tw weighted", "weighted", "padded", (), 2.0, "k_anneal_csr_rank1_pair<16, tw>"),
    ("K2p weighted", "weighted", "padded", (("k2_tw", 2),), 2.0, "k_anneal_csr_rank1_pair<16>"),
    ("K2 weighted", "weighted", "padded", (("k2_pair", 2),), 2.0, "k_anneal_csr_rank1<16, 2>"),
    # K2's byte and bit state (MI_K2_STATE; without a threshold wavefront: more than 1024 replicas)
    ("K2 byte", "pair", None, (("k2_pair", 0),), 0.5, "k_anneal_csr_rank1<16, 1>"),
    ("K2 bit", "pair", None, (("k2_pair", 0),), 0.5, "k_anneal_csr_rank1<16, 0>"),
    ("K2 bit weighted", "weighted", "padded", (("k2_pair", 2),), 2.0, "k_anneal_csr_rank1<16, 0>"),
])
def test_structured_kernels(case, kind, order, options, beta, kernel, monkeypatch):
    force_k2_state(monkeypatch, case)
    rp, col, val, lin, c, w = csr_model(kind)
    X, E = cs.enumerate_binary(rowptr=rp, col=col, val=val, lin=lin, c_pair=c, weights=w)
    pi = cs.reference(E, beta, R)
    with Problem.csr_rank1(rp, col, val, lin, c, order=order, weights=w) as p:
        st, en, acc, name, wall = sample(p, beta, 3, options=options)
        sites = device_order(p, 9)
    report("csr %s %s order=%s" % (case, kind, order), name, R, wall)
    assert name == kernel, name
    cs.judge("2b %s %s beta=%g" % (name, kind, beta), cs.binary_index(st), en, E, pi, 1e-9, acc,
             cs.accept_moments_binary(E, 9, beta, pi, sites=sites))


@pytest.mark.parametrize("case,block,options,r_call,kernel", [
    ("K2w one slot", 64, (("k2_split", 1),), 256, "k_anneal_csr_rank1_wide<16, 1, tw>"),
    ("K2s one wavefront", 64, (("k2_split", 1), ("k2_tw", 2)), 256, "k_anneal_csr_rank1_split<16, 1>"),
    ("K2w two slots", 128, (("k2_split", 1),), 256, "k_anneal_csr_rank1_wide<16, 2, tw>"),
    ("K2w two slots, no tw", 128, (("k2_split", 1), ("k2_tw", 2)), 256, "k_anneal_csr_rank1_wide<16, 2>"),
    ("K2s two wavefronts", 128, (("k2_split", 1), ("k2_wide", 2)), 256, "k_anneal_csr_rank1_split<16, 2>"),
    ("K2 few reads", 64, (("k2_split", 2), ("k2_pair", 2)), 512, "k_anneal_csr_rank1<16, 2>"),
    ("K2 three waves", 64, (("k2_split", 2), ("k2_pair", 2), ("k2_waves", 3)), 510, "k_anneal_csr_rank1<16, 2>"),
    ("K2p tw", 64, (("k2_pair", 1),), 2048, "k_anneal_csr_rank1_pair<16, tw>"),
    # K2's byte and bit state beside a threshold wavefront (MI_K2_STATE; up to 1024 replicas a call)
    ("K2 byte tw", 64, (("k2_split", 2), ("k2_pair", 2)), 1024, "k_anneal_csr_rank1<16, 1, tw>"),
    ("K2 bit tw", 64, (("k2_split", 2), ("k2_pair", 2)), 1024, "k_anneal_csr_rank1<16, 0, tw>"),
])
def test_few_replica_structured_kernels(case, block, options, r_call, kernel, monkeypatch):
    """The forms the library picks by read count: 2^15 samples over calls of ``r_call`` replicas, 64-state model."""
    force_k2_state(monkeypatch, case)
    rp, col, val, lin, c = csr6()
    beta = 0.5
    X, E = cs.enumerate_binary(rowptr=rp, col=col, val=val, lin=lin, c_pair=c)
    total = (R_FEW // r_call) * r_call
    pi = cs.reference(E, beta, total)
    with Problem.csr_rank1(rp, col, val, lin, c, order="padded", block=block) as p:
        st, en, acc, name, wall = sample(p, beta, 9, r_call=r_call, total=total, options=options)
        sites = device_order(p, 6)
    report("csr few %s" % case, name, r_call, wall)
    assert name == kernel, name
    cs.judge("2b %s beta=%g" % (name, beta), cs.binary_index(st), en, E, pi, 1e-9, acc,
             cs.accept_moments_binary(E, 6, beta, pi, sites=sites))


# ---- Potts ---------------------------------------------------------------------------------------------------------------
MODELS = {"unit": lambda n: potts_model(n), "x2": lambda n: potts_model(n, 2.0), "hub": lambda n: hub_model()}


@pytest.mark.parametrize("case,n,K,beta,order,options,r_call,total,min_size,kernel", [
    ("K3", 6, 3, 0.5, None, (), R, R, 0, "k_anneal_potts<16>"),
    ("K3", 6, 3, 3.0, None, (), R, R, 0, "k_anneal_potts<16>"),
    ("K3 padded", 8, 2, 1.0, "padded", (("k3_fast", 2),), R, R, 0, "k_anneal_potts<16>"),
    ("K3f KM=8", 6, 3, 0.5, "padded", (), R, R, 0, "k_anneal_potts_fast<16, 8>"),
    ("K3f KM=8", 6, 3, 3.0, "padded", (), R, R, 0, "k_anneal_potts_fast<16, 8>"),
    ("K3f KM=8", 8, 2, 1.0, "padded", (), R, R, 0, "k_anneal_potts_fast<16, 8>"),
    ("K3f KM=8", 4, 5, 1.0, "padded", (), R, R, 0, "k_anneal_potts_fast<16, 8>"),
    ("K3f KM=16", 3, 9, 1.0, "padded", (), R, R, 0, "k_anneal_potts_fast<16, 16>"),
    ("K3f KM=8 tw", 3, 4, 1.0, "padded", (), 1024, R_FEW, 0, "k_anneal_potts_fast<16, 8, tw>"),
    ("K3f KM=16 tw", 2, 9, 1.0, "padded", (), 1024, R_FEW, 0, "k_anneal_potts_fast<16, 16, tw>"),
    ("K3f min_size", 6, 3, 0.5, "padded", (("min_cluster_size", 1),), R, R, 1, "k_anneal_potts_fast<16, 8>"),
    ("K3 min_size", 6, 3, 0.5, None, (("min_cluster_size", 1),), R, R, 1, "k_anneal_potts<16>"),
    # the model of the CPU file's Potts power check (couplings doubled): a case with proven power, held to the rule
    ("x2 K3f KM=8", 8, 2, 2.0, "padded", (), R, R, 0, "k_anneal_potts_fast<16, 8>"),
    ("x2 K3", 8, 2, 2.0, None, (), R, R, 0, "k_anneal_potts<16>"),
    # 32 adjacency entries: chain_stats.hub_model (18 variables, one with 17 neighbours; 64 labelings carry the mass)
    ("hub K3f D=32", 18, 2, 1.0, "padded", (), R, R, 0, "k_anneal_potts_fast<32, 8>"),
    ("hub K3f D=32 tw", 18, 2, 1.0, "padded", (), 1024, R_FEW, 0, "k_anneal_potts_fast<32, 8, tw>"),
    ("hub K3 D=32", 18, 2, 1.0, None, (), R, R, 0, "k_anneal_potts<32>"),
])
def test_potts_kernels(case, n, K, beta, order, options, r_call, total, min_size, kernel):
    rp, col, val, c = MODELS[case.split()[0] if case.split()[0] in MODELS else "unit"](n)
    L, E = cs.enumerate_potts(rp, col, val, c, n, K)
    pi = cs.reference(E, beta, total, cs.potts_allowed(L, K, min_size) if min_size else None)
    # a hard size bound needs a feasible start: labels i mod K
    init = np.tile((np.arange(n) % K).astype(np.uint16), (r_call, 1)) if min_size else None
    with Problem.potts_csr(rp, col, val, c, n, K, order=order) as p:
        lab, en, acc, name, wall = sample(p, beta, 5, r_call=r_call, total=total, init=init, options=options)
        sites = device_order(p, n)
    report("potts %s n=%d K=%d" % (case, n, K), name, r_call, wall)
    assert name == kernel, name
    cs.judge("2c %s n=%d K=%d min=%d beta=%g" % (name, n, K, min_size, beta), cs.potts_index(lab, K), en, E, pi, 1e-9, acc,
             cs.accept_moments_potts(E, n, K, beta, pi, min_size=min_size, sites=sites))


NODE_W = np.array([1, 2, 3, 1, 4, 2])
C_NODE = 3.0 / 32.0                       # c * w_i is exact in fp32: the chain's cw_i w-sums are the model's c w_i W


def weighted_problem(order, c=C_NODE):
    rp, col, val, _ = potts_model(6)
    cw = (np.float32(c) * NODE_W).astype(np.float32)
    return Problem.potts_csr(rp, col, val, c, 6, 3, order=order, energy_model=(val.astype(np.float64), c),
                             node_weights=(NODE_W.astype(np.int32), cw, NODE_W.astype(np.float64)))


@pytest.mark.parametrize("order,options,beta,kernel", [
    ("padded", (), 1.0, "k_anneal_potts_fast<16, 8, weighted>"),
    ("padded", (), 2.0, "k_anneal_potts_fast<16, 8, weighted>"),
    (None, (), 1.0, "k_anneal_potts<16, weighted>"),
])
def test_node_weight_kernels_chain_2d(order, options, beta, kernel):
    rp, col, val, _ = potts_model(6)
    L, E = cs.enumerate_potts(rp, col, val, C_NODE, 6, 3, node_weights=NODE_W)
    pi = cs.reference(E, beta, R)
    with weighted_problem(order) as p:
        lab, en, acc, name, wall = sample(p, beta, 5, options=options)
        sites = device_order(p, 6)
    report("potts node weights order=%s" % order, name, R, wall)
    assert name == kernel, name
    cs.judge("2d %s beta=%g" % (name, beta), cs.potts_index(lab, 3), en, E, pi, 1e-9, acc,
             cs.accept_moments_potts(E, 6, 3, beta, pi, sites=sites))


def test_two_resolution_groups_each_sample_their_own_model():
    """Two groups of 2^17 replicas in one launch, pair coefficients c and 2 c, each at its own beta: group g is judged
    against the enumeration of ITS coefficient."""
    rp, col, val, _ = potts_model(6)
    cs_g, betas = [C_NODE, 2 * C_NODE], [1.0, 2.0]
    refs = []
    for c, beta in zip(cs_g, betas):
        L, E = cs.enumerate_potts(rp, col, val, c, 6, 3, node_weights=NODE_W)
        refs.append((E, cs.reference(E, beta, R // 2)))
    with weighted_problem("padded") as p:
        cw = np.stack([(np.float32(c) * NODE_W).astype(np.float32) for c in cs_g])
        p.set_node_weight_groups(cw, cs_g, [0.0, 0.0])
        lab, en, acc, name, wall = sample(p, None, 5, betas=betas)
        sites = device_order(p, 6)
    report("potts two resolution groups", name, R, wall)
    assert name == "k_anneal_potts_fast<16, 8, weighted>", name
    mean = var = 0.0
    for g, (c, beta) in enumerate(zip(cs_g, betas)):
        E, pi = refs[g]
        sl = slice(g * (R // 2), (g + 1) * (R // 2))
        cs.judge("2d group %d c=%g beta=%g" % (g, c, beta), cs.potts_index(lab[sl], 3), en[sl], E, pi, 1e-9)
        m = cs.accept_moments_potts(E, 6, 3, beta, pi, sites=sites)
        mean, var = mean + m[0] / 2, var + m[1] / 2
    # the accepted count of the launch is the sum over both groups: R / 2 replicas with each group's moments
    z = cs.accept_z(acc, R, mean, var)
    print("    accepted moves of both groups: %+.2f s.e." % z)
    assert abs(z) <= cs.Z_MAX


def test_merge_moves_are_rejected_as_a_sampler():
    """Chain 2e on the device, as in the CPU file: with a merge phase before every sweep the (6, 3) case is REJECTED
    (p < 1e-12); merges serve optimisation, not sampling."""
    n, K, beta = 6, 3, 0.5
    rp, col, val, c = potts_model(n)
    L, E = cs.enumerate_potts(rp, col, val, c, n, K)
    with Problem.potts_csr(rp, col, val, c, n, K, order="padded") as p:
        p.set_merge_moves(1, 2 * K)
        p.anneal(R, np.full(40, beta), 5)
        lab, en, _ = p.fetch()
        name, merges = p.kernel_name(), p.merges_accepted()
    assert name == "k_anneal_potts_fast<16, 8> + k_potts_merge", name
    x2, df, pv, pooled, bins = cs.chi_square(np.bincount(cs.potts_index(lab, K), minlength=len(E)), cs.boltzmann(E, beta))
    print("    2e %s: chi2 %.1f / %d  p %.3g  (%d merges)" % (name, x2, df, pv, merges))
    assert merges > 0 and pooled <= cs.POOL_MAX and pv < cs.P_REJECT


# ---- tempering -------------------------------------------------------------------------------------------------------------
def test_device_tempering_keeps_every_rung_at_its_own_temperature():
    """tempering_begin / anneal(betas=None, num_sweeps=1) / tempering_exchange (K6), 4 rungs x 2^16 chains, 41 rounds:
    the states that hold rung k are Boltzmann at beta_k (the CPU file explains why that pins the exchange rule)."""
    Qs = cs.random_dense(6, 106)
    X, E = cs.enumerate_binary(Qs=Qs)
    for beta in PT_LADDER:
        cs.reference(E, beta, PT_CHAINS)
    t0 = time.perf_counter()
    with Problem.dense(Qs) as p:
        out = tempering.parallel_tempering(tempering.ProblemEngine(p, 13), PT_LADDER, chains=PT_CHAINS, rounds=41,
                                           sweeps_per_round=1, seed=13, history=False)
        name = p.kernel_name()
        # one further sweep at the temperatures resident on the device (the rungs after the last exchange): its
        # accepted moves against the rungs' moments -- the only independent hold on the per-replica-beta path's counters
        p.anneal(4 * PT_CHAINS, None, 13, sweep_offset=41, continue_run=True, num_sweeps=1)
        assert p.kernel_name() == name
        accepted = p.fetch(states=False)[2]["accepted"]
    report("tempering 4 x 2^16", name, 4 * PT_CHAINS, time.perf_counter() - t0)
    assert name == "k_anneal_dense_wg<4,4>", name
    assert 0.05 < out["swap_rate"] < 0.95
    judge_rungs("pt " + name, out["local_states"], out["energies"], out["rung"], E, 1e-4, accepted=accepted)
