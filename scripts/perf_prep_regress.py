"""``select_regressed`` (the regression of covariates out of the chosen genes, csrc/prep_kernels.hip) beside the plain
``select`` on the same handle, and ``cell_qc``, in one run:
  (a) PBMC3k-shaped: 2638 cells x 13 714 genes of Poisson counts (the generator of scripts/perf_prep.py), the 2000 genes
      with the most non-zero cells, one covariate (the cell's percent of counts in the first tenth of the genes);
  (b) 50 000 cells x 4096 genes, all of them features, 8 covariates (seven standard normal columns and that percent).
Kernel milliseconds are HIP event times of the pass's kernels only, the median over --reps launches after one warm-up
launch, the two passes alternating.  ``select_regressed`` runs the gather, then four passes that read Z (coefficients, the
sum and the centred squares of the residuals, the scaling) and one that writes it; the traffic model is the gather's
(n x h f32 read from the n x g matrix, n x ldz f32 written) plus five times n x ldz f32, and ``achieved_gb_per_s`` is that
model over the measured time (Q and the per-gene vectors are left out: at most 72 bytes per cell and pass).  The wall time
of the host QR of the design is recorded too.  No threshold: the numbers are recorded.  Prints one JSON document (and writes
--out).

    python scripts/perf_prep_regress.py --reps 5 --out profiles/prep_regress.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scrna_seq_qannealing_clustering_amd import _lib, preprocess  # noqa: E402


def counts(rng, n, g, log_rate=-2.5):
    rate = np.exp(rng.normal(log_rate, 1.5, g))
    depth = rng.uniform(0.5, 2.0, n)
    X = np.empty((n, g), dtype=np.float32)
    for i0 in range(0, n, 4096):
        X[i0:i0 + 4096] = rng.poisson(rate[None, :] * depth[i0:i0 + 4096, None])
    return X


def shape(rng, reps, n, g, h, p, log_rate):
    X = counts(rng, n, g, log_rate)
    ldz = (h + 127) // 128 * 128
    res = {"n": n, "genes": g, "features": h, "ldz": ldz, "covariates": p, "nonzero_share": float((X != 0).mean())}
    with preprocess.ExpressionMatrix(X) as m:
        m.normalize()
        qc_ms = []
        for rep in range(reps + 1):
            n_count, _, subset = m.cell_qc(np.arange(g) < max(g // 10, 1))
            if rep:
                qc_ms.append(m.timing["qc_ms"])
        res["cell_qc"] = {"ms": qc_ms, "median_ms": float(np.median(qc_ms)),
                          "achieved_gb_per_s": 4.0 * n * g / (np.median(qc_ms) * 1e-3) / 1e9}
        percent = 100.0 * subset / np.where(n_count > 0, n_count, 1.0)
        cov = np.column_stack([rng.normal(size=(n, p - 1)), percent])
        t0 = time.perf_counter()
        Q, _ = preprocess.design_basis(cov, n=n)
        res["design_qr_s"] = time.perf_counter() - t0
        mean, var, cnt = m.gene_stats("normalized")
        genes = np.sort(np.argsort(-cnt, kind="stable")[:h]).astype(np.int32)
        plain, regressed = [], []
        for rep in range(reps + 1):
            m.select(genes, mean[genes], np.sqrt(var[genes]), 10.0)
            m.select_regressed(genes, Q, 10.0)
            if rep:
                plain.append(m.timing["select_ms"])
                regressed.append(m.timing["regress_ms"])
        res["flat_columns"] = int(m.flat.sum())
    gather = 4.0 * n * (h + ldz)
    res["select"] = {"ms": plain, "median_ms": float(np.median(plain)), "model_bytes": gather,
                     "achieved_gb_per_s": gather / (np.median(plain) * 1e-3) / 1e9}
    model = gather + 5 * 4.0 * n * ldz
    res["select_regressed"] = {"ms": regressed, "median_ms": float(np.median(regressed)), "model_bytes": model,
                               "achieved_gb_per_s": model / (np.median(regressed) * 1e-3) / 1e9}
    res["regressed_over_select"] = res["select_regressed"]["median_ms"] / res["select"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    out = {"reps": args.reps, "device": _lib.device_info(0)}
    out["pbmc3k_shape_2000_features_1_covariate"] = shape(rng, args.reps, 2638, 13714, 2000, 1, -2.5)
    print("pbmc3k_shape", json.dumps(out["pbmc3k_shape_2000_features_1_covariate"]), flush=True)
    out["50000x4096_features_8_covariates"] = shape(rng, args.reps, 50000, 4096, 4096, 8, -1.0)
    s = json.dumps(out, indent=1)
    print(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
