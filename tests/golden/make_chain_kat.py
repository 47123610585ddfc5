#!/usr/bin/env python3
"""Freeze one trajectory of every annealing chain into tests/golden/chain_kat.json.

A PR THAT REGENERATES chain_kat.json CHANGES THE CHAIN SPECIFICATION AND MUST SAY SO: the file
was written by the oracle as it stood before the tests that read it existed (the round-3 Potts rounding -- one signed
fp32 sum for the field difference -- is the pinned one), and tests/test_chain_kat.py holds today's oracle and the
kernels to it.

One entry per chain -- 2a dense, 2b structured, 2b with pair-term weights, 2c Potts, 2c with a minimum cluster size,
2d node weights, 2e merge moves, and a tempering run whose two exchange steps pin K6 -- on the 40-node breadth-first
subgraph of the committed noisy_circles graph: 8 replicas x 25 sweeps of the default geometric schedule, one seed.
Each entry holds the SHA-256 of the state bytes, the accepted count, the energies as hex floats and the first
replica's state spelled out (so a diff is readable).  ``cases()`` builds the models and runs the CPU side; the tests
import it, so generator and test cannot drift apart.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

from conftest import load_fixture  # noqa: E402

OUT = os.path.join(HERE, "chain_kat.json")
R, S, SEED, NODES = 8, 25, 20261, 40
LADDER = [0.5, 1.0, 2.0, 4.0]           # tempering entry: 2 chains x 4 rungs, 3 rounds of 5 sweeps, 2 exchange steps


def f32(a):
    return np.asarray(a, dtype=np.float32)


def bfs_nodes(fx, start, count):
    """The first ``count`` nodes of a breadth-first search, neighbours in adjacency order (as make_kat.py's; restated here
    so that importing this module -- the GPU test does -- loads nothing of the oracle)."""
    adj = {v: [] for v in fx.nodes}
    for u, v, _ in fx.edges:
        adj[u].append(v)
        adj[v].append(u)
    seen, order, queue = {start}, [start], [start]
    while queue and len(order) < count:
        cur = queue.pop(0)
        for nb in adj[cur]:
            if nb not in seen:
                seen.add(nb)
                order.append(nb)
                queue.append(nb)
                if len(order) == count:
                    break
    return order


def subgraph():
    """The subgraph induced by the first 40 nodes of a breadth-first search from the first node of noisy_circles."""
    from scrna_seq_qannealing_clustering_amd.graphs import graph_from_edges
    fx = load_fixture("noisy_circles")
    nodes = bfs_nodes(fx, fx.nodes[0], NODES)
    idx = {fx.nodes.index(v): k for k, v in enumerate(nodes)}
    keep = [k for k, (a, b) in enumerate(zip(fx.eu.tolist(), fx.ev.tolist())) if a in idx and b in idx]
    eu = [idx[int(fx.eu[k])] for k in keep]
    ev = [idx[int(fx.ev[k])] for k in keep]
    return graph_from_edges(nodes, eu, ev, fx.w[keep])


def weighted_layout(rowptr, col, weights):
    """Seats of a model with pair-term weights as ``Problem.csr_rank1(order="padded", weights=...)`` lays it out: the
    unit-weight variables in edge-free 64-seat slots, the others in one more slot.  Returns (seats, n_dev)."""
    from scrna_seq_qannealing_clustering_amd.models import padded_slot_layout
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    deg = np.diff(rowptr)
    light, heavy = np.flatnonzero(weights == 1), np.flatnonzero(weights != 1)
    renum = np.full(len(weights), -1, dtype=np.int64)
    renum[light] = np.arange(len(light))
    rp_l = np.concatenate([[0], np.cumsum(deg[light])]).astype(np.int32)
    seats_l, nslots, _ = padded_slot_layout(rp_l, renum[col[np.repeat(weights == 1, deg)]].astype(np.int32), slot=64)
    seats = np.empty(len(weights), dtype=np.int64)
    seats[light] = seats_l
    seats[heavy] = nslots * 64 + np.arange(len(heavy))
    return seats, (nslots + 1) * 64


def models_of_the_cases():
    """The inputs of every entry (shared by the generator, the CPU test and the GPU test)."""
    from scrna_seq_qannealing_clustering_amd import models
    from scrna_seq_qannealing_clustering_amd.sampler import default_potts_beta_range
    G = subgraph()
    m = models.build_bqm_qubo(G, 0.05)
    c = float(np.float32(m.c_pair))
    out = {"bqm": m, "betas": models.make_beta_schedule(S, models.default_beta_range(m)),
           "Qs": np.ascontiguousarray(m.dense_Qs().astype(np.float32)),
           "csr": (m.rowptr, m.col, f32(m.val), f32(m.lin), c)}
    # 2b weighted: two slack-like variables of weight 2 and 4 without couplings behind the 40
    n = m.num_variables
    w = np.array([1] * n + [2, 4], dtype=np.int64)
    rp = np.concatenate([m.rowptr, [m.rowptr[-1]] * 2]).astype(np.int32)
    lin = np.concatenate([f32(m.lin), f32([-3.0 * c, -9.0 * c])])
    out["csr_w"] = (rp, m.col, f32(m.val), lin, c, w)
    pm = models.build_dqm_potts(G, 4, 0.005)
    out["potts"] = pm
    out["potts_args"] = (pm.rowptr, pm.col, f32(pm.val), float(np.float32(pm.c_pair)), pm.num_variables, 4)
    out["potts_betas"] = models.make_beta_schedule(S, default_potts_beta_range(pm))
    mm = models.build_modularity_potts(G, 1.0, 6)
    out["mod"] = mm
    out["mod_betas"] = models.make_beta_schedule(S, models.modularity_beta_range(mm))
    return out


def raw(states, accepted, energies, **extra):
    return np.ascontiguousarray(states), int(accepted), np.asarray(energies, dtype=np.float64), extra


def entry(states, accepted, energies, **extra):
    states = np.ascontiguousarray(states)
    e = {"shape": list(states.shape), "dtype": str(states.dtype), "sha256": hashlib.sha256(states.tobytes()).hexdigest(),
         "accepted": int(accepted), "energies_hex": [float(x).hex() for x in energies],
         "first_replica": "".join("%x" % int(x) for x in states[0])}
    e.update(extra)
    return e


def cases(which=None):
    """{name: entry} of the CPU side of every chain (``which``: a subset of names)."""
    return {k: entry(*v[:3], **v[3]) for k, v in run_cases(which).items()}


def run_cases(which=None, replica_offset=0, replicas=R):
    """Run the CPU side of every chain (``which``: a subset of names) for the replicas ``replica_offset ..
    replica_offset + replicas - 1``; returns {name: (states, accepted, energies, extra fields of the entry)}."""
    from oracle import sa_oracle as so
    from scrna_seq_qannealing_clustering_amd import models, tempering
    from test_modularity_model import chain2d, device_energies
    from test_potts_merge_model import chain2e
    from test_tempering import OracleEngine
    M = models_of_the_cases()
    ro, Rn = replica_offset, replicas
    want = (lambda k: which is None or k in which)
    out = {}
    if want("2a"):
        st, en, stats = so.sa_dense_philox(M["Qs"], Rn, M["betas"], SEED, replica_offset=ro)
        out["2a"] = raw(st, stats[1], en)
    if want("2b"):
        st, en, stats = so.sa_csr_rank1_philox(*M["csr"], Rn, M["betas"], SEED, replica_offset=ro)
        out["2b"] = raw(st, stats[1], en)
    if want("2b_weighted"):
        rp, col, val, lin, c, w = M["csr_w"]
        seats, n_dev = weighted_layout(rp, col, w)
        prp, pcol, pval = models.pad_csr(rp, col, val, seats, n_dev)
        plin = np.full(n_dev, np.inf, dtype=np.float32)
        plin[seats] = lin
        pw = np.ones(n_dev, dtype=np.int32)
        pw[seats] = w
        st, en, stats = so.sa_csr_rank1_philox(prp, pcol, f32(pval), plin, c, Rn, M["betas"], SEED, replica_offset=ro,
                                               weights=pw)
        out["2b_weighted"] = raw(st[:, seats], stats[1], en, seats=[int(x) for x in seats], n_dev=int(n_dev))
    pm = M["potts"]
    for name, ms in (("2c", 0), ("2c_min_size", 6)):
        if want(name):
            lab, en, stats = so.potts_csr_philox(*M["potts_args"], Rn, M["potts_betas"], SEED, lin_offset=pm.lin_offset,
                                                 replica_offset=ro, min_size=ms)
            out[name] = raw(lab, stats[1], en, min_size=ms)
    mm = M["mod"]
    if want("2d") or want("2e"):
        wq, cw, w64 = models.potts_node_weights(mm)
        v32 = f32(mm.val)
        hole = np.zeros(mm.num_variables, dtype=bool)

        def energies(lab):
            return device_energies(np.asarray(mm.rowptr, dtype=np.int64), np.asarray(mm.col, dtype=np.int64), mm.val, w64,
                                   mm.c_pair, mm.lin_offset, lab, hole, mm.num_cases)
    if want("2d"):
        lab, acc, _ = chain2d(mm.rowptr, mm.col, v32, wq, cw, mm.num_cases, Rn, M["mod_betas"], SEED, replica_offset=ro)
        out["2d"] = raw(lab, acc, energies(lab))
    if want("2e"):
        cq = float(models.potts_merge_coefficients(mm)[0])
        lab, acc, merges = chain2e(mm.rowptr, mm.col, v32, wq.astype(np.int64), cw, cq, mm.num_cases, Rn, M["mod_betas"],
                                   SEED, 4, 2 * mm.num_cases, replica_offset=ro)
        out["2e"] = raw(lab, acc, energies(lab), merges=int(merges), merge_interval=4, proposals=2 * mm.num_cases)
    if want("k6_exchange") and ro == 0 and Rn == R:
        eng = OracleEngine("dense", (M["Qs"],), SEED)
        pt = tempering.parallel_tempering(eng, np.asarray(LADDER), chains=R // len(LADDER), rounds=3, sweeps_per_round=5,
                                          seed=SEED, history=False)
        rung, proposed, accepted = eng.rungs()
        out["k6_exchange"] = raw(pt["local_states"], accepted, pt["energies"], rung=[int(x) for x in rung],
                                   proposed=int(proposed))
    return out


def main():
    out = {"replicas": R, "sweeps": S, "seed": SEED, "nodes": NODES, "ladder": LADDER, "entries": cases()}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True)[:2000])


if __name__ == "__main__":
    main()
