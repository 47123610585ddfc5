"""Label agreement on the device against its floors and the host:
  (a) replica stability of the 8-resolution sweep (gamma = 0.2 .. 1.6, 256 reads each, K = 16, bench graph) on the
      states in HBM (Problem.label_agreement, 8 x C(256, 2) pairs) against the anneal's own kernel time;
  (b) all pairs of 4096 labellings at n = 2638, K = 16 (C(4096, 2) pairs, 5.8e12 i8 MACs): kernel time and the share of
      the i8 MFMA floor (16x16x64: 16 cycles per SIMD, 256 CUs x 4 SIMDs, at the clock the caller gives);
  (c) the host: a vectorised numpy bincount contingency per pair, on a sample of pairs of (b), per-pair cost.
Kernel milliseconds from HIP events, median over --reps after a warm-up; prints one JSON document (and writes --out).

    python scripts/perf_agreement.py --reps 5 --out profiles/agreement_stability_and_all_pairs.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from scrna_seq_qannealing_clustering_amd import metrics, models  # noqa: E402
from scrna_seq_qannealing_clustering_amd.engine import Problem  # noqa: E402


def host_pair(a, b, Kb, n):
    t = np.bincount(a * Kb + b, minlength=Kb * Kb)
    S = int((t * (t - 1) // 2).sum())
    nz = t[t > 0].astype(np.float64)
    return S, float((nz * np.log(nz)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=16000)
    ap.add_argument("--labellings", type=int, default=4096)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"reps": args.reps}

    # (a) the sweep's replica stability
    G = bench.build_workload()[4]
    gammas = [round(0.2 * (g + 1), 10) for g in range(8)]
    pms = models.build_modularity_sweep(G, gammas, 16)
    betas = np.stack([models.make_beta_schedule(args.sweeps, models.modularity_beta_range(pm)) for pm in pms])
    wq, cw, w64, c64, offset = models.potts_node_weight_groups(pms)
    pm = pms[0]
    with Problem.potts_csr(pm.rowptr, pm.col, pm.val.astype(np.float32), float(np.float32(pm.c_pair)), pm.num_variables,
                           pm.num_cases, lin_offset=pm.lin_offset, order="padded", energy_model=(pm.val, pm.c_pair),
                           node_weights=models.potts_node_weights(pm)) as p:
        p.set_node_weight_groups(cw, c64, offset)
        p.anneal(8 * 256, betas, 1)
        anneal_ms = p.kernel_ms()
        ms = []
        for rep in range(args.reps + 1):
            r = p.label_agreement()
            if rep:
                ms.append(r["kernel_ms"])
        labels, _, _ = p.fetch()
    stab = [float(np.mean(r["ari"][g])) for g in range(8)]
    t0 = time.perf_counter()
    sample = [(i, j) for i in range(0, 256, 16) for j in range(i + 1, 256, 16)]
    for i, j in sample:
        host_pair(labels[i].astype(np.int64), labels[j].astype(np.int64), 16, labels.shape[1])
    host_pair_us = (time.perf_counter() - t0) / len(sample) * 1e6
    out["sweep_stability"] = {"gammas": gammas, "reads": 256, "sweeps": args.sweeps, "anneal_kernel_ms": anneal_ms,
                              "agreement_kernel_ms": ms, "agreement_median_ms": float(np.median(ms)),
                              "share_of_anneal": float(np.median(ms)) / anneal_ms, "mean_ari_per_gamma": stab,
                              "host_numpy_us_per_pair": host_pair_us,
                              "host_numpy_s_all_pairs": host_pair_us * 1e-6 * 8 * 256 * 255 / 2}

    # (b) all pairs of many labellings near a 9-cluster truth
    rng = np.random.default_rng(0)
    n, R, K = 2638, args.labellings, 16
    truth = rng.integers(0, 9, n)
    L = np.tile(truth, (R, 1))
    flip = rng.random((R, n)) < 0.1
    L[flip] = rng.integers(0, K, int(flip.sum()))
    L[0, 0] = K - 1
    ms = []
    for rep in range(args.reps + 1):
        r = metrics.label_agreement(L)
        if rep:
            ms.append(r["kernel_ms"])
    pairs = R * (R - 1) // 2
    npad = (n + 63) // 64 * 64
    macs = pairs * 16 * 16 * npad
    floor_ms = pairs * (npad // 64) * 16 / (256 * 4 * args.clock_ghz * 1e9) * 1e3
    out["all_pairs"] = {"labellings": R, "n": n, "K": K, "pairs": pairs, "i8_macs_padded": macs,
                        "kernel_ms": ms, "median_ms": float(np.median(ms)),
                        "mfma_floor_ms_at_clock": floor_ms, "clock_ghz_assumed": args.clock_ghz,
                        "fraction_of_floor": floor_ms / float(np.median(ms)),
                        "mac_per_s": macs / (float(np.median(ms)) * 1e-3)}
    t0 = time.perf_counter()
    idx = rng.integers(0, R, (2000, 2))
    for i, j in idx:
        host_pair(L[i], L[j], K, n)
    us = (time.perf_counter() - t0) / len(idx) * 1e6
    out["all_pairs"]["host_numpy_us_per_pair"] = us
    out["all_pairs"]["host_numpy_s_all_pairs"] = us * 1e-6 * pairs
    out["host_threads"] = 1
    s = json.dumps(out, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
