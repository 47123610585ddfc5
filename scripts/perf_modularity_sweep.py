"""A resolution sweep in one grouped launch against the same runs one after another, on the bench graph, in one process,
the two alternating: gamma = 0.2, 0.4, ..., 1.6 (8 groups: 2048 replicas, K3f without its threshold wavefront) and the
first four of them (4 groups: 1024 replicas, with it), 256 reads x 16000 sweeps per resolution, K = 16, each resolution
on its own modularity_beta_range -- the defaults of clustering_modularity(_sweep).  Kernel milliseconds per repetition;
prints one JSON document (and writes it to --out).

    python scripts/perf_modularity_sweep.py --reps 3 --out profiles/modularity_sweep_grouped_vs_sequential.json
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


def make_problem(pm):
    return Problem.potts_csr(pm.rowptr, pm.col, pm.val.astype(np.float32), float(np.float32(pm.c_pair)),
                             pm.num_variables, pm.num_cases, lin_offset=pm.lin_offset, order="padded",
                             energy_model=(pm.val, pm.c_pair), node_weights=models.potts_node_weights(pm))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reads", type=int, default=256)
    ap.add_argument("--sweeps", type=int, default=16000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    G = bench.build_workload()[4]
    rows = []
    for ngroups in (8, 4):
        gammas = [round(0.2 * (g + 1), 10) for g in range(ngroups)]
        pms = models.build_modularity_sweep(G, gammas, 16)
        betas = np.stack([models.make_beta_schedule(args.sweeps, models.modularity_beta_range(pm)) for pm in pms])
        wq, cw, w64, c64, offset = models.potts_node_weight_groups(pms)
        grouped = make_problem(pms[0])
        grouped.set_node_weight_groups(cw, c64, offset)
        singles = [make_problem(pm) for pm in pms]
        R = args.reads
        ms = {"grouped": [], "sequential": []}
        per_gamma = [[] for _ in pms]
        names = {}
        same = True
        for rep in range(args.reps + 1):                           # rep 0: warm-up
            for k in ("grouped", "sequential") if rep % 2 == 0 else ("sequential", "grouped"):
                if k == "grouped":
                    grouped.anneal(ngroups * R, betas, 100 + rep)
                    lab_g, en_g, _ = grouped.fetch()
                    t = grouped.kernel_ms()
                    names[k] = grouped.kernel_name()
                else:
                    t = 0.0
                    lab_s, en_s = [], []
                    for g, p in enumerate(singles):
                        p.anneal(R, betas[g], 100 + rep)
                        lab, en, _ = p.fetch()
                        lab_s.append(lab)
                        en_s.append(en)
                        t += p.kernel_ms()
                        if rep:
                            per_gamma[g].append(p.kernel_ms())
                    names[k] = singles[0].kernel_name()
                if rep:
                    ms[k].append(t)
            same = same and np.array_equal(lab_g, np.concatenate(lab_s)) and np.array_equal(en_g, np.concatenate(en_s))
        best_q = [float(-en_g[g * R:(g + 1) * R].min() / pm.info["m"]) for g, pm in enumerate(pms)]
        grouped.close()
        for p in singles:
            p.close()
        row = {"groups": ngroups, "resolutions": gammas, "reads_per_group": R, "sweeps": args.sweeps, "K": 16,
               "grouped_equals_sequential": bool(same), "best_modularity": best_q,
               "per_resolution_median_ms": [float(np.median(x)) for x in per_gamma]}
        for k in ms:
            row[k] = {"kernel": names[k], "ms": ms[k], "median_ms": float(np.median(ms[k])),
                      "spread_ms": float(np.max(ms[k]) - np.min(ms[k]))}
        row["speedup_sequential_over_grouped"] = row["sequential"]["median_ms"] / row["grouped"]["median_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    doc = {"graph": "bench.build_workload synthetic_snn (n = 2638)", "reps": args.reps, "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
