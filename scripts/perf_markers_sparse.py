"""The rank-sum marker pass on a resident ExpressionMatrix (mi_prep_rank_sum_markers) beside the dense entry point
(mi_rank_sum_markers_f32 on a host array), in one session on one device:
  (a) PBMC3k-shaped: n = 2638 cells, g = 13 714 genes, about 6 % non-zero, K = 9, for B = 1 and B = 8 labellings;
  (b) kidney-shaped: n = 10 605, g = 21 063, K = 15, B = 1;
  (c) n = 50 000, g = 20 000 at 6 %, K = 15, B = 1: sparse only (dense it is 4 GB on the host and 8 GB on the device).
Expression as in scripts/perf_markers.py: a Bernoulli mask times log1p of a small count, generated in column slabs and kept
as CSR.  At each shape, interleaved inside every repetition: the unchanged dense entry point (host scan, upload, transpose,
rank, sums), the dense handle (count, transpose, rank, sums on the resident matrix) and the sparse handle with both ways of
reading the values (``gather="inplace"``: V[pos[k]] in the kernels; ``gather="permute"``: one copy into gene-major order
first).  Kernel milliseconds from HIP events and wall milliseconds of the whole call, median over --reps after a warm-up;
the handles are created once, outside the timed calls (their creation time is recorded).  Every output of every handle form
is compared with the dense entry point's, bit for bit.  No threshold: the numbers are recorded.

    python scripts/perf_markers_sparse.py --reps 7 --out profiles/markers_sparse.json
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

from scrna_seq_qannealing_clustering_amd import metrics  # noqa: E402
from scrna_seq_qannealing_clustering_amd.preprocess import ExpressionMatrix  # noqa: E402

KEYS = ("rank2", "npos", "tie", "sum")


def expression_csr(rng, n, g, density):
    slabs = []
    for j0 in range(0, g, 2048):
        w = min(2048, g - j0)
        rows, cols = np.nonzero(rng.random((n, w), dtype=np.float32) < density)
        vals = np.log1p(1.7 * (1 + rng.poisson(0.8, len(rows)))).astype(np.float32)
        slabs.append(sp.csr_matrix((vals, (rows, cols)), shape=(n, w)))
    return sp.hstack(slabs, format="csr")


def summary(k, w):
    return {"kernel_ms": k, "kernel_median_ms": float(np.median(k)), "wall_ms": w, "wall_median_ms": float(np.median(w))}


def case(name, A, L, K, reps, dense=True):
    n, g = A.shape
    res = {"n": n, "genes": g, "labellings": int(L.shape[0]), "K": K, "stored_entries": int(A.nnz),
           "nonzero_share": A.nnz / (n * g), "max_stored_per_gene": int(np.diff(A.tocsc().indptr).max())}
    forms = {}
    handles = []
    X = None
    if dense:
        X = A.toarray()
        forms["dense_entry"] = lambda: metrics.rank_sum_pass(X, L, K)
        t0 = time.perf_counter()
        md = ExpressionMatrix(X)
        res["dense_handle_create_s"] = time.perf_counter() - t0
        handles.append(md)
        forms["dense_handle"] = lambda: md.rank_sum_pass(L, K, which="counts")
    t0 = time.perf_counter()
    ms = ExpressionMatrix(A)
    res["sparse_handle_create_s"] = time.perf_counter() - t0
    handles.append(ms)
    res["sparse_handle_device_bytes"] = ms.device_bytes()
    forms["sparse_handle_inplace"] = lambda: ms.rank_sum_pass(L, K, which="counts", gather="inplace")
    forms["sparse_handle_permute"] = lambda: ms.rank_sum_pass(L, K, which="counts", gather="permute")
    forms["sparse_handle_default"] = lambda: ms.rank_sum_pass(L, K, which="counts")
    times = {f: ([], []) for f in forms}
    last = {}
    for rep in range(reps + 1):
        for f, fn in forms.items():
            t0 = time.perf_counter()
            r = fn()
            wall = (time.perf_counter() - t0) * 1e3
            if rep:
                times[f][0].append(r["kernel_ms"])
                times[f][1].append(wall)
            last[f] = r
    for f in forms:
        res[f] = summary(*times[f])
    base = last["dense_entry"] if dense else last["sparse_handle_inplace"]
    res["outputs_equal_to"] = "dense_entry" if dense else "sparse_handle_inplace"
    res["outputs_equal"] = {f: bool(all(np.array_equal(last[f][k], base[k]) for k in KEYS)) for f in forms}
    n_ = np.int64(n)
    res["rank2_rows_add_up"] = bool((last["sparse_handle_default"]["rank2"].sum(axis=-1) == n_ * (n_ + 1)).all())
    if dense:
        e = res["dense_entry"]
        for f in ("dense_handle", "sparse_handle_inplace", "sparse_handle_permute"):
            res[f]["kernel_ratio_to_dense_entry"] = res[f]["kernel_median_ms"] / e["kernel_median_ms"]
            res[f]["wall_speedup_over_dense_entry"] = e["wall_median_ms"] / res[f]["wall_median_ms"]
    for m in handles:
        m.close()
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-kidney", action="store_true")
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks every shape (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    sc = lambda v: max(2, int(v * args.scale))
    out = {"reps": args.reps, "scale": args.scale, "lds_max_nonzeros": metrics.MARKERS_LDS_MAX_NONZEROS,
           "labelling_chunk": metrics.MARKERS_LABELLING_CHUNK}

    n, g = sc(2638), sc(13714)
    A = expression_csr(rng, n, g, 0.06)
    for B in (1, 8):
        out["pbmc3k_shape_B%d" % B] = case("pbmc3k_shape_B%d" % B, A, rng.integers(0, 9, (B, n)), 9, args.reps)
    if not args.skip_kidney:
        n, g = sc(10605), sc(21063)
        A = expression_csr(rng, n, g, 0.06)
        out["kidney_shape_B1"] = case("kidney_shape_B1", A, rng.integers(0, 15, (1, n)), 15, args.reps)
    if not args.skip_large:
        n, g = sc(50000), sc(20000)
        A = expression_csr(rng, n, g, 0.06)
        out["sparse_50000x20000_B1"] = case("sparse_50000x20000_B1", A, rng.integers(0, 15, (1, n)), 15, args.reps, dense=False)
    s = json.dumps(out, indent=1)
    print(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
