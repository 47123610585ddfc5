#!/usr/bin/env python3
"""Kernel times of the structured kernels the benchmark never runs, on the benchmark's graph (development helper): K2
(k2_split = 2, k2_pair = 2), K2s with one wavefront (k2_split = 1, k2_tw = 2) and K3 (k3_fast = 2), each at 1000 sweeps and
at 10 -- the short call is where the chain's ends (initial state, states out and fp64 energies) are the largest share.
Prints one JSON line: {arm: {sweeps: kernel_ms (median of --reps after one warm-up)}}.
usage: perf_chain_ends.py [--replicas R] [--reps K]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from scrna_seq_qannealing_clustering_amd import models  # noqa: E402
from scrna_seq_qannealing_clustering_amd.engine import Problem  # noqa: E402
from scrna_seq_qannealing_clustering_amd.sampler import default_potts_beta_range  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--replicas", type=int, default=500)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
m, _, _, _, graph = bench.build_workload()
n = m.num_variables
brange = models.default_beta_range(m)
pm = models.build_dqm_potts(graph, 8, 0.005)


def timed(p, betas, want):
    ms = []
    for rep in range(a.reps + 1):
        p.anneal(a.replicas, betas, 1234)
        p.fetch(states=False)
        ms.append(p.kernel_ms())
    assert want in p.kernel_name(), p.kernel_name()
    return float(np.median(ms[1:]))


out = {}
arms = (("k2", {"k2_split": 2, "k2_pair": 2}, "k_anneal_csr_rank1<"), ("k2s1", {"k2_split": 1, "k2_tw": 2}, "split<16, 1>"))
with Problem.csr_rank1(m.rowptr, m.col, m.val.astype(np.float32), m.lin.astype(np.float32), float(np.float32(m.c_pair)),
                       order="padded") as p:
    for arm, options, want in arms:
        for k in ("k2_split", "k2_pair", "k2_tw"):
            p.set_option(k, options.get(k, 0))
        out[arm] = {str(s): timed(p, models.make_beta_schedule(s, brange), want) for s in (1000, 10)}
        out[arm]["kernel"] = p.kernel_name()
with Problem.potts_csr(pm.rowptr, pm.col, pm.val.astype(np.float32), float(np.float32(pm.c_pair)), n, 8,
                       lin_offset=pm.lin_offset, order="padded") as p:
    p.set_option("k3_fast", 2)
    out["k3"] = {str(s): timed(p, models.make_beta_schedule(s, default_potts_beta_range(pm)), "k_anneal_potts<")
                 for s in (1000, 10)}
    out["k3"]["kernel"] = p.kernel_name()
print(json.dumps({"perf_chain_ends": out, "replicas": a.replicas, "reps": a.reps}))
