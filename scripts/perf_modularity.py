"""K3f with node weights (modularity, chain 2d) against K3f without (the DQM model) on the bench graph, in one process,
the two alternating: K = 8 and 16, 4096 reads x 200 sweeps and the sampler's default 256 x 1000, each model on its own
default schedule.  Prints one JSON document (and writes it to --out).

    python scripts/perf_modularity.py --reps 5 --out profiles/modularity_k3f_weighted_vs_unweighted.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from scrna_seq_qannealing_clustering_amd import models  # noqa: E402
from scrna_seq_qannealing_clustering_amd.engine import Problem  # noqa: E402
from scrna_seq_qannealing_clustering_amd.sampler import default_potts_beta_range  # noqa: E402


def make_problem(pm):
    return Problem.potts_csr(pm.rowptr, pm.col, pm.val.astype(np.float32), float(np.float32(pm.c_pair)),
                             pm.num_variables, pm.num_cases, lin_offset=pm.lin_offset, order="padded",
                             energy_model=(pm.val, pm.c_pair), node_weights=models.potts_node_weights(pm))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    G = bench.build_workload()[4]
    rows = []
    for K in (8, 16):
        pms = {"unweighted": models.build_dqm_potts(G, K, 0.005), "weighted": models.build_modularity_potts(G, 1.0, K)}
        for R, S in ((4096, 200), (256, 1000)):
            probs = {k: make_problem(pm) for k, pm in pms.items()}
            betas = {k: models.make_beta_schedule(S, default_potts_beta_range(pm)) for k, pm in pms.items()}
            ms = {k: [] for k in pms}
            acc = {}
            names = {}
            for rep in range(args.reps + 1):                       # rep 0: warm-up
                for k in ("unweighted", "weighted") if rep % 2 == 0 else ("weighted", "unweighted"):
                    p = probs[k]
                    p.anneal(R, betas[k], 100 + rep)
                    _, en, info = p.fetch(states=False)
                    if rep:
                        ms[k].append(p.kernel_ms())
                    acc[k] = info["accepted"] / info["proposals"]
                    names[k] = p.kernel_name()
                    if k == "weighted":
                        best_q = float(-en.min() / pms[k].info["m"])
            for p in probs.values():
                p.close()
            row = {"K": K, "reads": R, "sweeps": S, "best_modularity": best_q}
            for k in pms:
                row[k] = {"kernel": names[k], "ms": ms[k], "median_ms": float(np.median(ms[k])),
                          "spread_ms": float(np.max(ms[k]) - np.min(ms[k])), "acceptance": acc[k]}
            row["ratio_weighted_over_unweighted"] = row["weighted"]["median_ms"] / row["unweighted"]["median_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    doc = {"graph": "bench.build_workload synthetic_snn (n = 2638)", "reps": args.reps, "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
