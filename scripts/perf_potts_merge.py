"""Merge moves (chain 2e) on the bench graph at resolution 1: quality and kernel time of the modularity chain with and
without merge phases.  256 reads, K = 16 (K3f with its threshold wavefront) and K = 32 (K3), 1000 / 2000 / 4000 / 16000
sweeps geometric over models.modularity_beta_range (the driver's default schedule), without merges and with a merge
phase of 2 K proposals every M sweeps for each M of --intervals.  Per configuration and repetition (seed = repetition):
best and mean Q = -E / m over the reads, kernel milliseconds, launches, accepted merges; the variants of one row alternate
in one process.  Then the merge phase alone: 64 sweeps in one launch against the same 64 sweeps cut by a merge phase
before every sweep (63 phases), at 256 and 4096 reads.  Prints one JSON line per row and writes the document to --out.

    python scripts/perf_potts_merge.py --reps 3 --out profiles/potts_merge_quality_time.json
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


def run(p, pm, R, betas, seed, interval, proposals):
    p.set_merge_moves(interval, proposals, models.potts_merge_coefficients(pm))
    p.anneal(R, betas, seed)
    _, en, info = p.fetch(states=False)
    q = -en / pm.info["m"]
    return {"best_q": float(q.max()), "mean_q": float(q.mean()), "ms": p.kernel_ms(), "launches": p.launch_count(),
            "kernel": p.kernel_name(), "merges": p.merges_accepted(), "accepted": info["accepted"]}


def summary(runs):
    ms = [r["ms"] for r in runs]
    return {"best_q": [r["best_q"] for r in runs], "mean_q": [r["mean_q"] for r in runs], "ms": ms,
            "median_ms": float(np.median(ms)), "spread_ms": float(np.max(ms) - np.min(ms)),
            "median_best_q": float(np.median([r["best_q"] for r in runs])),
            "median_mean_q": float(np.median([r["mean_q"] for r in runs])),
            "launches": runs[0]["launches"], "kernel": runs[0]["kernel"],
            "merges_accepted": [r["merges"] for r in runs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reads", type=int, default=256)
    ap.add_argument("--Ks", default="16,32")
    ap.add_argument("--sweeps", default="1000,2000,4000,16000")
    ap.add_argument("--intervals", default="25,100")
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    G = bench.build_workload()[4]
    R = args.reads
    intervals = [int(x) for x in args.intervals.split(",")]
    rows, alone = [], []
    for K in [int(x) for x in args.Ks.split(",")]:
        pm = models.build_modularity_potts(G, 1.0, K)
        P = 2 * K
        p = make_problem(pm)
        run(p, pm, R, models.make_beta_schedule(200, models.modularity_beta_range(pm)), 0, intervals[0], P)   # warm-up
        for S in ([] if args.skip_quality else [int(x) for x in args.sweeps.split(",")]):
            betas = models.make_beta_schedule(S, models.modularity_beta_range(pm))
            variants = [0] + intervals
            res = {v: [] for v in variants}
            for rep in range(args.reps):
                for v in (variants if rep % 2 == 0 else variants[::-1]):
                    res[v].append(run(p, pm, R, betas, 1 + rep, v, P))
            row = {"K": K, "reads": R, "sweeps": S, "proposals": P}
            for v in variants:
                row["no_merges" if v == 0 else "M=%d" % v] = summary(res[v])
            rows.append(row)
            print(json.dumps(row), flush=True)
        # the merge phase alone: 64 sweeps, one launch, against the same sweeps with a phase before each of sweeps 1..63
        for Ra in (256, 4096):
            betas = models.make_beta_schedule(64, models.modularity_beta_range(pm))
            plain, cut = [], []
            for rep in range(args.reps + 1):
                a = run(p, pm, Ra, betas, 7, 0, P)
                b = run(p, pm, Ra, betas, 7, 1, P)
                if rep:
                    plain.append(a["ms"])
                    cut.append(b["ms"])
            row = {"K": K, "reads": Ra, "sweeps": 64, "one_launch_ms": plain, "with_63_phases_ms": cut,
                   "launches_with_phases": b["launches"],
                   "per_phase_ms": float((np.median(cut) - np.median(plain)) / 63.0),
                   "one_launch_per_sweep_ms": float(np.median(plain) / 64.0)}
            alone.append(row)
            print(json.dumps(row), flush=True)
        p.close()
    doc = {"graph": "bench.build_workload synthetic_snn (n = 2638), resolution 1", "reps": args.reps,
           "louvain_q": 0.8229, "rows": rows, "merge_phase_alone": alone}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
