"""Cell-type annotation on the device (annotate.single_r: mi_annot_create / _score / _fine_tune) against the CPU restatement
of tests/annot_reference.py, at the shape of the reference notebook's SingleR call:
  (a) PBMC3k-shaped: n = 2638 cells x 13 714 genes against a 114-sample reference (the Monaco shape) with L = 10 main and
      L = 29 fine labels;
  (b) 50 000 cells against the L = 10 reference (5 000 cells drawn, tiled tenfold: the device work per cell is the same).
Synthetic values: per label a profile with --up up-regulated genes (a third of the labels are near-twins of another, so
that fine-tuning iterates), log-normal reference samples, Poisson cells of --depth counts, log-normalised, held as CSR.
Per shape: kernel milliseconds per pass from HIP events (ranking the reference, ranking the cells, the MFMA cross pass,
the scores, fine-tuning) and wall milliseconds of the whole call (gene intersection, densify per chunk, upload, kernels,
download, pruning; the markers are computed once per reference and timed apart), median over --reps after a warm-up; and
the wall time of the restatement on the first --host-cells cells of the same input, whose labels, iteration counts and
scores the device's are compared with.  No threshold: the numbers are recorded.  Prints one JSON document (and writes --out).

    python scripts/perf_annotate.py --reps 3 --out profiles/annotate.json
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

import annot_reference as ar  # noqa: E402
from scrna_seq_qannealing_clustering_amd import annotate  # noqa: E402


def problem(rng, L, S, g, n, up, depth):
    base = rng.gamma(2.0, 0.4, g)
    prof = np.tile(base, (L, 1))
    for l in range(L):
        if l % 3 == 2:                                              # a near-twin of the label before it
            prof[l] = prof[l - 1]
            hit = rng.choice(g, up // 5, replace=False)
        else:
            hit = rng.choice(g, up, replace=False)
        prof[l, hit] += rng.uniform(1.0, 2.5, len(hit))
    ids = np.arange(S) % L
    R = (prof[ids] + rng.normal(0.0, 0.15, (S, g))).astype(np.float32)
    truth = rng.integers(0, L, n)
    blocks = []
    for i0 in range(0, n, 1000):                                    # in slabs: 2638 x 13 714 doubles at a time is enough
        rate = np.expm1(prof[truth[i0:i0 + 1000]])
        counts = rng.poisson(rate / rate.sum(axis=1, keepdims=True) * depth)
        blocks.append(sp.csr_matrix(np.log1p(counts / np.maximum(counts.sum(axis=1, keepdims=True), 1) * 1e4).astype(np.float32)))
    return sp.vstack(blocks).tocsr(), R, ["label_%02d" % l for l in ids], truth


def case(name, X, names, ref, truth, reps, host_cells):
    n = X.shape[0]
    res = {"cells": n, "genes": X.shape[1], "samples": ref.R.shape[0], "labels": ref.L, "de_n": ref.de_n,
           "nonzero_share": float(X.nnz / (X.shape[0] * X.shape[1]))}
    t0 = time.perf_counter()
    pairs, M = ref.markers_on(annotate.common_genes(names, ref.gene_names)[1])
    res["markers_host_s"] = time.perf_counter() - t0
    res["marker_genes"] = int(len(M))
    walls, kernels = [], []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        r = annotate.single_r(X, names, ref)
        if rep:
            walls.append((time.perf_counter() - t0) * 1e3)
            kernels.append(r["kernel_ms"])
    res["device"] = {"wall_ms": walls, "wall_median_ms": float(np.median(walls)),
                     "kernel_median_ms": {k: float(np.median([v[k] for v in kernels])) for k in kernels[0]}}
    res["iterations_histogram"] = np.bincount(r["iterations"]).tolist()
    res["accuracy_against_planted"] = float(np.mean(r["label_ids"] == truth))
    res["pruned"] = int(sum(v is None for v in r["pruned_labels"]))
    # the restatement on the first cells of the same input
    hc = min(host_cells, n)
    pos = {int(j): k for k, j in enumerate(M)}
    local = {ab: [pos[int(j)] for j in genes] for ab, genes in pairs.items()}
    XM = X[:hc][:, M].toarray()                                     # (the test's genes are the reference's here, in order)
    t0 = time.perf_counter()
    e = ar.annotate(XM, ref.R[:, M], ref.label_ids, ref.L, local)
    res["host_cells"] = hc
    res["restatement_s_sample"] = time.perf_counter() - t0
    res["restatement_s_all_cells_scaled"] = res["restatement_s_sample"] * n / hc
    clear = e["margin"] > 1e-6
    res["host_cells_with_clear_margin"] = int(clear.sum())
    res["labels_equal_on_sample"] = bool(np.array_equal(r["label_ids"][:hc][clear], e["labels"][clear])
                                         and np.array_equal(r["iterations"][:hc][clear], e["iterations"][clear]))
    res["scores_bit_identical_on_sample"] = bool(np.array_equal(r["scores"][:hc], e["scores"]))
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-cells", type=int, default=200)
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
    for L in (10, 29):
        X, R, labels, truth = problem(rng, L, 114, args.genes, args.cells, args.up, args.depth)
        ref = annotate.Reference(R, names, labels)
        out["pbmc3k_shape_L%d" % L] = case("pbmc3k_shape_L%d" % L, X, names, ref, truth, args.reps, args.host_cells)
        if L == 10 and args.big_cells:
            tile = -(-args.big_cells // 5000)
            Xb, Rb, lb, tb = problem(rng, L, 114, args.genes, -(-args.big_cells // tile), args.up, args.depth)
            Xb, tb = sp.vstack([Xb] * tile).tocsr()[:args.big_cells], np.tile(tb, tile)[:args.big_cells]
            out["cells_%d_L10" % args.big_cells] = case("cells_%d_L10" % args.big_cells, Xb, names,
                                                         annotate.Reference(Rb, names, lb), tb, args.reps, args.host_cells)
    s = json.dumps(out, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
