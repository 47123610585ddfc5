"""The rank-sum marker pass on the device (mi_rank_sum_markers_f32) against the host loop over the genes:
  (a) PBMC3k-shaped: n = 2638 cells, g = 13 714 genes, about 6 % non-zero, K = 9, for B = 1 and B = 8 labellings;
  (b) kidney-shaped: n = 10 605, g = 21 063, K = 15, B = 1;
  (c) a dense n = 50 000 slice of 256 genes (every cell non-zero: the HBM form of the ranking pass).
Expression: a Bernoulli mask times log1p of a small count (ties among the non-zeros, as in log-normalised data); (c) is
standard normal.  Beside each device number the time of the host loop (tests/markers_reference.py: scipy.stats.rankdata per
gene, np.add.at per labelling) on the first --host-genes genes of the same input, scaled to all genes; the device's
integers are compared with it on those genes.  Kernel milliseconds from HIP events (transpose, ranking and sums together)
and wall milliseconds of the whole call (host scan, upload, kernels, download), median over --reps after a warm-up.  No
threshold: the numbers are recorded.  Prints one JSON document (and writes --out).

    python scripts/perf_markers.py --reps 5 --out profiles/markers_rank_sum.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from markers_reference import reference_stats  # noqa: E402
from scrna_seq_qannealing_clustering_amd import metrics  # noqa: E402


def expression(rng, n, g, density):
    X = np.zeros((n, g), dtype=np.float32)
    for j0 in range(0, g, 2048):                                   # in slabs: the kidney shape is 223 M entries
        w = min(2048, g - j0)
        mask = rng.random((n, w), dtype=np.float32) < density
        X[:, j0:j0 + w] = mask * np.log1p(1.7 * (1 + rng.poisson(0.8, (n, w)))).astype(np.float32)
    return X


def timed(X, L, K, reps, force_global=False):
    k, w = [], []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        r = metrics.rank_sum_pass(X, L, K, force_global=force_global)
        if rep:
            k.append(r["kernel_ms"])
            w.append((time.perf_counter() - t0) * 1e3)
    return r, {"kernel_ms": k, "kernel_median_ms": float(np.median(k)), "wall_ms": w, "wall_median_ms": float(np.median(w))}


def case(name, X, L, K, reps, host_genes, force_global=False):
    n, g = X.shape
    res = {"n": n, "genes": g, "labellings": int(L.shape[0]), "K": K, "nonzero_share": float((X != 0).mean()),
           "max_nonzeros_per_gene": int((X != 0).sum(axis=0).max()), "force_global": force_global}
    r, res["device"] = timed(X, L, K, reps, force_global)
    hg = min(host_genes, g)
    t0 = time.perf_counter()
    rank2, npos, sums, tie, _ = reference_stats(X[:, :hg], L, K)
    host = time.perf_counter() - t0
    res["host_genes"] = hg
    res["host_loop_s_sample"] = host
    res["host_loop_s_all_genes_scaled"] = host * g / hg
    res["integers_equal_on_sample"] = bool(np.array_equal(r["rank2"][:, :hg], rank2) and np.array_equal(r["npos"][:, :hg], npos)
                                           and np.array_equal(r["tie"][:hg], tie))
    res["sums_max_rel_err_on_sample"] = float(np.max(np.abs(r["sum"][:, :hg] - sums) / np.maximum(np.abs(sums), 1e-300)))
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-genes", type=int, default=256)
    ap.add_argument("--skip-kidney", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    out = {"reps": args.reps, "lds_max_nonzeros": metrics.MARKERS_LDS_MAX_NONZEROS,
           "labelling_chunk": metrics.MARKERS_LABELLING_CHUNK, "host_threads": 1}

    X = expression(rng, 2638, 13714, 0.06)
    for B in (1, 8):
        L = rng.integers(0, 9, (B, 2638))
        out["pbmc3k_shape_B%d" % B] = case("pbmc3k_shape_B%d" % B, X, L, 9, args.reps, args.host_genes)
    if not args.skip_kidney:
        X = expression(rng, 10605, 21063, 0.06)
        out["kidney_shape_B1"] = case("kidney_shape_B1", X, rng.integers(0, 15, (1, 10605)), 15, args.reps, args.host_genes)
    X = rng.standard_normal((50000, 256), dtype=np.float32)
    out["dense_50000_hbm_form"] = case("dense_50000_hbm_form", X, rng.integers(0, 15, (1, 50000)), 15, args.reps,
                                       min(args.host_genes, 32), force_global=True)
    s = json.dumps(out, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
