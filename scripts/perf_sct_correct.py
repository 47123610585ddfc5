"""SCTransform's corrected counts (``ExpressionMatrix.sct_correct``, ``mi_prep_sct_correct``) on the device, per shape:
  - the kernel milliseconds of ``sct_correct`` (the gene table and, for a sparse handle, the count, scan and fill launches of
    the row pass and the counting sort that builds the transpose);
  - the yardstick: ``sct_residual_moments`` on the same handle in the same session -- the pass of the same arithmetic (one
    exp, one division, one square root per cell x gene, made twice) that the package already had;
  - the numpy fp64 restatement (tests/sct_correct_reference.py) on this machine's CPU, on all rows or, for the large shape,
    on the first --host-rows rows (recorded, with the time scaled to all rows beside it), and whether the device's corrected
    counts of those rows equal it;
  - the density of the output against the input's.
Shapes: PBMC3k's (2638 x 13 714; Poisson counts with per-gene rates exp(N(-2.5, 1.5)) and per-cell depth U(0.5, 2)) as a dense
and as a sparse handle, and 50 000 x 20 000 sparse at 6 % (multinomial draws over genes of log-normal abundance, a five-fold
range of depth).  The model is synthetic but plausible: every gene detected in 5 cells is listed, b1 ~ N(2.3, 0.3) (counts proportional to depth), b0 puts the gene's mean at the mean depth, alpha ~ U(0, 0.5),
the reference depth is log10 of the median total.  Kernel milliseconds are HIP event times, the median over --reps calls
after one warm-up call.  No threshold: the numbers are recorded.  Prints one JSON document (and writes --out).

    python scripts/perf_sct_correct.py --reps 5 --out profiles/prep_sct_correct.json
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

import sct_correct_reference as cr  # noqa: E402
from scrna_seq_qannealing_clustering_amd import _lib, preprocess  # noqa: E402


def poisson_counts(rng, n, g, log_rate=-2.5):
    rate = np.exp(rng.normal(log_rate, 1.5, g))
    depth = rng.uniform(0.5, 2.0, n)
    X = np.empty((n, g), dtype=np.float32)
    for i0 in range(0, n, 4096):
        X[i0:i0 + 4096] = rng.poisson(rate[None, :] * depth[i0:i0 + 4096, None])
    return X


def sparse_counts(rng, n, g, per_cell):
    """multinomial counts: a cell draws per_cell / 3 .. 5 per_cell / 3 molecules (a five-fold range of depth, so that cells lie
    on both sides of the reference depth; per_cell on average), each from the genes with probabilities proportional to
    exp(N(0, 1.5)); a gene's count is the number of its draws.  1480 draws per cell leave 6 % of 20 000 genes non-zero."""
    prob = np.exp(rng.normal(0.0, 1.5, g))
    cdf = np.cumsum(prob / prob.sum())
    draws = rng.integers(per_cell // 3, 2 * per_cell - per_cell // 3 + 1, n)
    total = int(draws.sum())
    cols = np.minimum(np.searchsorted(cdf, rng.random(total)), g - 1).astype(np.int32)
    A = sp.coo_matrix((np.ones(total, dtype=np.float32), (np.repeat(np.arange(n, dtype=np.int32), draws), cols)), shape=(n, g)).tocsr()
    A.sum_duplicates()
    return A


def model(rng, A):
    """-> (genes, b0, b1, alpha, log_umi, log_umi_ref) from the counts (a csr_matrix)"""
    n, g = A.shape
    total = np.asarray(A.sum(axis=1), dtype=np.float64).ravel()
    lu = np.log10(total)
    detected = np.asarray((A != 0).sum(axis=0)).ravel()
    genes = np.flatnonzero(detected >= 5).astype(np.int32)
    mean = np.asarray(A.sum(axis=0), dtype=np.float64).ravel()[genes] / n
    b1 = rng.normal(2.3, 0.3, len(genes))
    b0 = np.log(mean) - b1 * lu.mean()
    alpha = rng.uniform(0.0, 0.5, len(genes))
    return genes, b0, b1, alpha, lu, float(np.log10(np.median(total)))


def measure(name, M, A, par, reps, host_rows):
    genes, b0, b1, alpha, lu, lu_ref = par
    n, g = A.shape
    res = {"handle": name, "n": n, "genes": g, "listed_genes": int(len(genes)), "input_nnz": int((A.data != 0).sum()),
           "input_density": float((A.data != 0).sum() / (n * g))}
    rows = n if host_rows is None else min(n, host_rows)
    with preprocess.ExpressionMatrix(M) as m:
        res["source_device_bytes"] = m.device_bytes()
        correct_ms, moments_ms = [], []
        for rep in range(reps + 1):
            out = m.sct_correct(genes, b0, b1, alpha, lu, lu_ref)
            m.sct_residual_moments(genes, b0, b1, alpha, lu)
            if rep:
                correct_ms.append(m.timing["sct_correct_ms"])
                moments_ms.append(m.timing["sct_moments_ms"])
            if rep < reps:
                out.close()
        res["sct_correct"] = {"ms": correct_ms, "median_ms": float(np.median(correct_ms))}
        res["sct_residual_moments"] = {"ms": moments_ms, "median_ms": float(np.median(moments_ms))}
        res["correct_over_moments"] = res["sct_correct"]["median_ms"] / res["sct_residual_moments"]["median_ms"]
        with out:
            res["output_device_bytes"] = out.device_bytes()
            counts = out.fetch_counts()
            nnz = int(counts.nnz) if out.sparse else int((counts != 0).sum())
            res["output_nnz"], res["output_density"] = nnz, nnz / (n * g)
            got = (counts[:rows].toarray() if out.sparse else counts[:rows])[:, genes]
    block = np.asarray(A[:rows][:, genes].todense(), dtype=np.float32)
    t0 = time.perf_counter()
    v = cr.values(block, b0, b1, alpha, lu[:rows], lu_ref)
    want = cr.count_of(v)
    data = cr.data_slot(want)
    host_s = time.perf_counter() - t0
    res["host_numpy_fp64"] = {"rows": rows, "seconds": host_s, "seconds_scaled_to_all_rows": host_s * n / rows,
                              "threads_env": os.environ.get("OMP_NUM_THREADS")}
    near = cr.near_half(v)
    res["equals_restatement_on_those_rows"] = bool(np.array_equal(got[~near], want[~near].astype(np.float32)))
    res["entries_within_1e-9_of_a_half_integer"] = int(near.sum())
    res["zero_to_count"], res["count_to_zero"] = int(((block == 0) & (want != 0)).sum()), int(((block != 0) & (want == 0)).sum())
    del data
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-rows", type=int, default=4096, help="rows of the large shape the numpy restatement is timed on")
    ap.add_argument("--large", default="50000x20000x1480", help="cells x genes x draws per cell of the large sparse shape")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    out = {"reps": args.reps, "device": _lib.device_info(0), "host_cpus_usable": len(os.sched_getaffinity(0)), "shapes": []}
    X = poisson_counts(rng, 2638, 13714)
    X = X[X.sum(axis=1) > 0]
    A = sp.csr_matrix(X)
    par = model(rng, A)
    for name, M in (("dense", X), ("sparse", A)):
        out["shapes"].append(measure("pbmc3k_shape_" + name, M, A, par, args.reps, None))
        print(json.dumps(out["shapes"][-1]), flush=True)
    a, b = out["shapes"][0], out["shapes"][1]
    out["pbmc3k_sparse_nnz_equals_dense"] = a["output_nnz"] == b["output_nnz"]
    n, g, per_cell = (int(v) for v in args.large.split("x"))
    A = sparse_counts(rng, n, g, per_cell)
    out["shapes"].append(measure("sparse_%dx%d" % (n, g), A, A, model(rng, A), args.reps, args.host_rows))
    s = json.dumps(out, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
