"""Co-association (consensus) on the device against its floor and the host:
  (a) M2 + M3 in place (Problem.coassociation: histogram and the model's edges) after the 8-resolution sweep (gamma =
      0.2 .. 1.6, 256 reads each, K = 16, bench graph) against the anneal's own kernel time; the row-sum passes
      that `consensus=True` adds for the per-cell confidence, apart and in the total;
  (b) M2 for 4096 reads at n = 2638, K = 8 and K = 16 (both padded to 16 label rows): kernel time, MAC/s and the share
      of the i8 MFMA floor (16x16x64: 16 cycles per SIMD, 256 CUs x 4 SIMDs, at the clock the caller gives -- an
      estimate), over the tiles on and above the diagonal of the 128-cell block grid;
  (c) the host restatement (C += (L[r][:, None] == L[r][None, :]) per read, bincount of the upper triangle) on a sample
      of the reads of the same inputs, scaled to all of them;
  (d) with --loop: the per-round numbers of clustering_consensus on the bench graph (what was observed, no claim).
Kernel milliseconds from HIP events, median over --reps after a warm-up; prints one JSON document (and writes --out).

    python scripts/perf_consensus.py --reps 5 --out profiles/consensus_coassociation.json
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
from scrna_seq_qannealing_clustering_amd import clustering, metrics, models  # noqa: E402
from scrna_seq_qannealing_clustering_amd.engine import Problem  # noqa: E402
from scrna_seq_qannealing_clustering_amd.sampler import model_edges  # noqa: E402


def host_restatement_s(L, sample):
    """seconds for the numpy restatement over `sample` reads of L, and for its histogram"""
    n = L.shape[1]
    Cm = np.zeros((n, n), dtype=np.int64)
    t0 = time.perf_counter()
    for r in range(sample):
        Cm += L[r][:, None] == L[r][None, :]
    t1 = time.perf_counter()
    np.bincount(Cm[np.triu_indices(n, 1)], minlength=L.shape[0] + 1)
    return (t1 - t0) / sample, time.perf_counter() - t1


def median_ms(fn, reps):
    ms = []
    for rep in range(reps + 1):
        r = fn()
        if rep:
            ms.append(r["kernel_ms"])
    return ms, float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=16000)
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"reps": args.reps}

    # (a) after the default sweep, in place
    G = bench.build_workload()[4]
    gammas = [round(0.2 * (g + 1), 10) for g in range(8)]
    pms = models.build_modularity_sweep(G, gammas, 16)
    betas = np.stack([models.make_beta_schedule(args.sweeps, models.modularity_beta_range(pm)) for pm in pms])
    wq, cw, w64, c64, offset = models.potts_node_weight_groups(pms)
    pm = pms[0]
    eu, ev = model_edges(pm)
    with Problem.potts_csr(pm.rowptr, pm.col, pm.val.astype(np.float32), float(np.float32(pm.c_pair)), pm.num_variables,
                           pm.num_cases, lin_offset=pm.lin_offset, order="padded", energy_model=(pm.val, pm.c_pair),
                           node_weights=models.potts_node_weights(pm)) as p:
        p.set_node_weight_groups(cw, c64, offset)
        p.anneal(8 * 256, betas, 1)
        anneal_ms = p.kernel_ms()
        both, both_med = median_ms(lambda: p.coassociation(edges=(eu, ev)), args.reps)
        m2, m2_med = median_ms(lambda: p.coassociation(), args.reps)
        m3, m3_med = median_ms(lambda: p.coassociation(edges=(eu, ev), hist=False), args.reps)
        res = p.coassociation(edges=(eu, ev))
        labs = [metrics.consensus_labels(res["edge_counts"][g], 256, eu, ev, pm.num_variables) for g in range(8)]
        passes = [metrics.confidence_passes(l) for l in labs]
        ref = np.stack([ps[0][0] if ps else np.zeros(pm.num_variables, dtype=np.int64) for ps in passes])
        rs, rs_med = median_ms(lambda: p.coassociation(ref=ref, hist=False), args.reps)
        npass = max(len(ps) for ps in passes)
        labels, _, _ = p.fetch()
    per_read, hist_s = host_restatement_s(labels[:256], 32)
    out["after_sweep"] = {
        "gammas": gammas, "reads": 256, "sweeps": args.sweeps, "n": int(pm.num_variables), "edges": int(len(eu)),
        "anneal_kernel_ms": anneal_ms, "hist_and_edges_kernel_ms": both, "hist_and_edges_median_ms": both_med,
        "share_of_anneal": both_med / anneal_ms, "dense_only_median_ms": m2_med, "edges_only_median_ms": m3_med,
        "rowsum_pass_median_ms": rs_med, "rowsum_passes_for_cell_confidence": npass,
        "consensus_true_total_ms": both_med + npass * rs_med,
        "consensus_true_share_of_anneal": (both_med + npass * rs_med) / anneal_ms, "pac_per_gamma": [metrics.pac(res["hist"][g]) for g in range(8)],
        "consensus_clusters_per_gamma": [int(l.max()) + 1 for l in labs],
        "host_numpy_s_all_groups": 8 * (per_read * 256 + hist_s)}

    # (b) many reads, dense pass only
    rng = np.random.default_rng(0)
    n, R = 2638, args.reads
    nb = (n + 127) // 128
    tiles = nb * (nb + 1) // 2
    out["many_reads"] = {}
    for K in (8, 16):
        truth = rng.integers(0, min(K, 9), n)
        L = np.tile(truth, (R, 1))
        flip = rng.random((R, n)) < 0.1
        L[flip] = rng.integers(0, K, int(flip.sum()))
        L[0, 0] = K - 1
        ms, med = median_ms(lambda: metrics.coassociation(L), args.reps)
        mfmas = tiles * 64 * (R // 4)                       # 8 x 8 MFMA tiles of 16 x 16 per block tile, 4 reads x 16 label rows per k-step
        macs = mfmas * 16 * 16 * 64
        floor_ms = mfmas * 16 / (256 * 4 * args.clock_ghz * 1e9) * 1e3
        per_read, hist_s = host_restatement_s(L, 16)
        out["many_reads"]["K%d" % K] = {
            "reads": R, "n": n, "K": K, "label_rows_padded": 16, "block_tiles": tiles, "i8_macs_padded": macs,
            "useful_macs": n * (n - 1) // 2 * R * K, "kernel_ms": ms, "median_ms": med,
            "mfma_floor_ms_at_clock_estimate": floor_ms, "clock_ghz_assumed": args.clock_ghz,
            "fraction_of_floor": floor_ms / med, "mac_per_s": macs / (med * 1e-3),
            "host_numpy_s": per_read * R + hist_s}

    if args.loop:
        ss = clustering.clustering_consensus(G, 1.0, 16, max_rounds=5, sampler_kwargs=dict(seed=1, num_sweeps=args.sweeps))
        out["consensus_loop"] = {"resolution": 1.0, "tau": 0.5, "seed": 1, "sweeps": args.sweeps,
                                 "rounds": ss.info["consensus_rounds"], "converged": ss.info["consensus_converged"],
                                 "history": ss.info["consensus_history"],
                                 "best_read_modularity_last_round": float(np.max(ss.info["modularity"]))}
    out["host_threads"] = 1
    s = json.dumps(out, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
