"""Annotation on the resident expression handle against today's host-array call, at the two shapes of profiles/annotate.json
(scripts/perf_annotate.py's synthetic generator, the same seed: 2638 x 13 714 and 50 000 x 13 714 cells, a 114-sample
reference with L = 10), in one process:
  host      annotate.single_r on the scipy CSR matrix (densify the marker columns per chunk on the host, upload, kernels)
  dense     single_r on an open dense ExpressionMatrix holding the same values (which="counts": the uploaded values)
  sparse    single_r on an open sparse ExpressionMatrix
  clusters  single_r(handle, clusters=...) with K = 9 clusters (the planted types, the last two merged), on both handles
Opening the handles is not timed: they are resident in the workflows this serves (after normalize() or sctransform()).
Per path: wall milliseconds of the whole call (median of --reps after a warm-up call), kernel milliseconds per pass, the
handle's device_bytes before and after, and whether the labels equal the host path's.  No threshold: the numbers and the
ratios host / path are recorded.  Prints one JSON document (and writes --out).

    python scripts/perf_annotate_resident.py --reps 3 --out profiles/annotate_resident.json
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from perf_annotate import problem  # noqa: E402
from scrna_seq_qannealing_clustering_amd import annotate, preprocess  # noqa: E402


def timed(call, reps):
    walls, kernels, r = [], [], None
    for rep in range(reps + 1):                                     # the first call is the warm-up
        t0 = time.perf_counter()
        r = call()
        if rep:
            walls.append((time.perf_counter() - t0) * 1e3)
            kernels.append(r["kernel_ms"])
    return r, {"wall_ms": walls, "wall_median_ms": float(np.median(walls)),
               "kernel_median_ms": {k: float(np.median([v[k] for v in kernels])) for k in kernels[0]}}


def case(name, X, names, ref, truth, reps):
    n = X.shape[0]
    res = {"cells": n, "genes": X.shape[1], "samples": ref.R.shape[0], "labels": ref.L,
           "nonzero_share": float(X.nnz / (X.shape[0] * X.shape[1]))}
    t0 = time.perf_counter()
    cols, _ = annotate._marker_setup(names, ref)
    res["marker_setup_host_ms_first_call"] = (time.perf_counter() - t0) * 1e3
    res["marker_genes"] = int(len(cols))
    clusters = np.minimum(truth, 8)
    host, res["host"] = timed(lambda: annotate.single_r(X, names, ref), reps)
    first_clusters = None
    for kind in ("dense", "sparse"):
        t0 = time.perf_counter()
        with preprocess.ExpressionMatrix(X.toarray() if kind == "dense" else X) as h:
            opened = time.perf_counter() - t0
            before = h.device_bytes()
            r, t = timed(lambda: annotate.single_r(h, names, ref, which="counts"), reps)
            t.update(open_handle_s_not_timed=opened, device_bytes_before=before, device_bytes_after=h.device_bytes(),
                     equals_host_path=bool(all(np.array_equal(r[k], host[k]) for k in ("label_ids", "scores", "iterations"))),
                     host_over_path=res["host"]["wall_median_ms"] / t["wall_median_ms"])
            res[kind] = t
            r, t = timed(lambda: annotate.single_r(h, names, ref, which="counts", clusters=clusters), reps)
            if first_clusters is None:
                first_clusters = r
            t.update(K=int(len(r["cluster_values"])), device_bytes_after=h.device_bytes(),
                     cluster_labels=[str(v) for v in r["labels"]],
                     equals_other_handle=bool(np.array_equal(r["scores"], first_clusters["scores"])),
                     host_over_path=res["host"]["wall_median_ms"] / t["wall_median_ms"])
            res["clusters_" + kind] = t
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--genes", type=int, default=13714)
    ap.add_argument("--cells", type=int, default=2638)
    ap.add_argument("--big-cells", type=int, default=50000, help="0 skips the large run")
    ap.add_argument("--up", type=int, default=120)
    ap.add_argument("--depth", type=float, default=2500.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    names = ["g%05d" % j for j in range(args.genes)]
    out = {"reps": args.reps, "max_chunk": annotate.MAX_CHUNK, "host_threads": 1}
    L = 10
    X, R, labels, truth = problem(rng, L, 114, args.genes, args.cells, args.up, args.depth)
    out["pbmc3k_shape_L10"] = case("pbmc3k_shape_L10", X, names, annotate.Reference(R, names, labels), truth, args.reps)
    if args.big_cells:
        tile = -(-args.big_cells // 5000)
        Xb, Rb, lb, tb = problem(rng, L, 114, args.genes, -(-args.big_cells // tile), args.up, args.depth)
        Xb, tb = sp.vstack([Xb] * tile).tocsr()[:args.big_cells], np.tile(tb, tile)[:args.big_cells]
        out["cells_%d_L10" % args.big_cells] = case("cells_%d_L10" % args.big_cells, Xb, names, annotate.Reference(Rb, names, lb),
                                                     tb, args.reps)
    s = json.dumps(out, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
