"""``preprocess.sctransform`` stage by stage (csrc/prep_kernels.hip: the gene attributes, the negative-binomial fit, the
residual moments, the residual selection, then the Gram / project kernels every chain shares), in one run:
  (a) PBMC3k-shaped: 2638 cells x 13 714 genes, dense, all cells and 2000 genes in the fit, 3000 features, one covariate (the
      cell's percent of counts in the first tenth of the genes), 50 PCs; the numpy fp64 restatement of the same chain
      (tests/sct_reference.py) is timed on the same machine;
  (b) 50 000 cells x 20 000 genes as a ``scipy.sparse`` matrix, 5000 cells and 2000 genes in the fit, 3000 features, the same
      covariate (the restatement is not run: it would need the dense fp64 matrix, 8 GB).
Counts are Poisson(rate_j * depth_i * exp(s_j z_i)): a log-normal depth (sigma 0.5) and a per-cell factor z that gene j
follows with strength s_j ~ U(0, 0.7), so that most genes are overdispersed about their depth trend.  Kernel milliseconds are
HIP event times of the pass's kernels only, the median over --reps runs of the driver after one warm-up run; ``wall_s`` is the
driver end to end (upload included).  For the fit the rounds per gene and the share of genes converged are recorded.  No
threshold: the numbers are recorded.  Prints one JSON document (and writes --out).

    python scripts/perf_sct.py --reps 5 --out profiles/prep_sct.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from scrna_seq_qannealing_clustering_amd import _lib, preprocess  # noqa: E402

KERNELS = ("qc_ms", "gene_stats_counts_ms", "gene_log1p_ms", "nb_fit_ms", "sct_moments_ms", "sct_select_ms", "gram_ms",
           "project_ms")
HOST = ("sct_subsample_s", "sct_regularize_s", "eigh_s")


def counts(rng, n, g, log_rate, sparse):
    rate = np.exp(rng.normal(log_rate, 1.5, g))
    strength = rng.uniform(0.0, 0.7, g)
    depth = np.exp(rng.normal(0.0, 0.5, n))
    z = rng.normal(size=n)
    blocks = []
    for i0 in range(0, n, 2048):
        lam = rate[None, :] * depth[i0:i0 + 2048, None] * np.exp(strength[None, :] * z[i0:i0 + 2048, None])
        B = rng.poisson(lam).astype(np.float32)
        B[B.sum(axis=1) == 0, 0] = 1.0                           # (no cell without counts)
        blocks.append(sp.csr_matrix(B) if sparse else B)
    return sp.vstack(blocks).tocsr() if sparse else np.vstack(blocks)


def percent_of_first_tenth(X):
    g = X.shape[1]
    first = np.asarray(X[:, :max(g // 10, 1)].sum(axis=1)).ravel()
    return 100.0 * first / np.asarray(X.sum(axis=1)).ravel()


def shape(rng, reps, n, g, log_rate, sparse, ncells, restate):
    X = counts(rng, n, g, log_rate, sparse)
    cov = percent_of_first_tenth(X)
    kw = dict(variable_features_n=3000, npcs=50, vars_to_regress=cov, ncells=ncells, n_genes=2000)
    res = {"n": n, "genes": g, "sparse": bool(sparse), "nonzero_share": float(X.nnz / (n * g)) if sparse else float((X != 0).mean()),
           "fit_cells": min(n, ncells), "features": 3000, "covariates": 1}
    runs, wall = [], []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        r = preprocess.sctransform(X, **kw)
        if rep:
            wall.append(time.perf_counter() - t0)
            runs.append(r.timing)
    for key in KERNELS + HOST:
        v = [t[key] for t in runs]
        res[key.rsplit("_", 1)[0]] = {"values": v, "median_" + key.rsplit("_", 1)[1]: float(np.median(v))}
    res["all_kernels_median_ms"] = float(np.median([sum(t[k] for k in KERNELS) for t in runs]))
    res["wall_s"] = {"values": wall, "median_s": float(np.median(wall))}
    it = r.model.iterations
    res["fit"] = {"genes": int(len(it)), "converged_share": float(r.model.converged.mean()),
                  "poisson_share": float(r.model.poisson.mean()), "rounds_median": float(np.median(it)),
                  "rounds_max": int(it.max()), "rounds_mean": float(it.mean()), "outliers": int(r.model.outlier.sum()),
                  "passing_genes": int(r.gene_attr.passing.sum())}
    if restate:
        import sct_reference
        t0 = time.perf_counter()
        w = sct_reference.sctransform(X, **kw)
        res["restatement_numpy_fp64_s"] = time.perf_counter() - t0
        res["restatement_same_genes"] = bool(set(w["genes"].tolist()) == set(r.genes.tolist()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small-only", action="store_true", help="the PBMC3k shape alone")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    out = {"reps": args.reps, "device": _lib.device_info(0)}
    out["pbmc3k_shape_dense"] = shape(rng, args.reps, 2638, 13714, -2.5, False, 5000, True)
    print("pbmc3k_shape", json.dumps(out["pbmc3k_shape_dense"]), flush=True)
    if not args.small_only:
        out["50000x20000_sparse"] = shape(rng, args.reps, 50000, 20000, -3.0, True, 5000, False)
    s = json.dumps(out, indent=1)
    print(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
