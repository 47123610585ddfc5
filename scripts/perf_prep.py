"""The preprocessing front end (preprocess.py, csrc/prep_kernels.hip) on the device against the same chain in numpy / scipy
fp64 on the host, in one run:
  (a) PBMC3k-shaped: 2638 cells x 13 714 genes of Poisson counts (per-gene rates exp(N(-2.5, 1.5)), per-cell depth U(0.5, 2)),
      2000 variable features, 50 PCs: every kernel's milliseconds and the end-to-end seconds of ``embed`` (upload, kernels,
      the host loess and eigen-solve, downloads);
  (b) 50 000 cells x 2000 features: the Gram and projection kernels alone, and the Gram kernel's share of the f32-input MFMA
      peak (157.3 TF), counted on the multiplications it executes (the upper block triangle; a diagonal tile skips a quarter).
Kernel milliseconds are HIP event times of the kernels only, the median over --reps launches after one warm-up launch; wall
times are the median over --reps calls after one warm-up call.  The host chain (tests/prep_reference.py, the same
``loess_fit``, ``scipy.linalg.eigh`` with the same subset) runs with the BLAS threads the environment grants
(OMP_NUM_THREADS is recorded).  No threshold: the numbers are recorded.  Prints one JSON document (and writes --out).

    python scripts/perf_prep.py --reps 5 --out profiles/prep_embed.json

``--sparse`` measures the sparse handle instead (``ExpressionMatrix`` of a ``scipy.sparse`` matrix) against the dense one in
the same process:
  (c) PBMC3k-shaped at 6 % non-zero (the same generator with its rates shifted down): per pass the kernel milliseconds of
      both handles, alternating; the wall time of the constructor of each, and of the sparse one's host part alone (the
      checks and the transpose of csrc/mi_prep_csr.h, compiled here with g++ -O3 into a scratch library and timed through
      ctypes; the rest of the constructor is allocation and upload); ``embed`` end to end on both; and that every output
      compared is identical;
  (d) 70 000 cells x 65 536 genes (4.6e9 entries: the dense handle refuses the shape) at about 1 % non-zero, built directly
      as CSR: the same passes, the constructor, and the bytes the handle holds on the device.

    python scripts/perf_prep.py --sparse --reps 5 --out profiles/prep_sparse.json
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import prep_reference as ref  # noqa: E402
from scrna_seq_qannealing_clustering_amd import _lib, preprocess  # noqa: E402

PEAK_F32_MFMA_TF = 157.3


def counts(rng, n, g, log_rate=-2.5):
    rate = np.exp(rng.normal(log_rate, 1.5, g))
    depth = rng.uniform(0.5, 2.0, n)
    X = np.empty((n, g), dtype=np.float32)
    for i0 in range(0, n, 4096):
        X[i0:i0 + 4096] = rng.poisson(rate[None, :] * depth[i0:i0 + 4096, None])
    return X


def median_ms(m, key, call, reps):
    out = []
    for rep in range(reps + 1):
        call()
        if rep:
            out.append(m.timing[key])
    return {"ms": out, "median_ms": float(np.median(out))}


def wall(call, reps):
    out = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        r = call()
        if rep:
            out.append(time.perf_counter() - t0)
    return r, {"s": out, "median_s": float(np.median(out))}


def gram_flops(n, h):
    """multiply-adds x 2 the Gram kernel executes: 128 x 128 tiles of the upper block triangle over all cells (rounded up
    to steps of 32), three quarters of a diagonal tile"""
    T = (h + 127) // 128
    steps = sum((min(n, c + preprocess.GRAM_CHUNK) - c + 31) // 32 for c in range(0, n, preprocess.GRAM_CHUNK))
    return 2.0 * 128 * 128 * 32 * steps * (T * (T - 1) / 2 + 0.75 * T)


def pbmc_shape(rng, reps, nfeatures, npcs):
    n, g = 2638, 13714
    X = counts(rng, n, g)
    res = {"n": n, "genes": g, "nonzero_share": float((X != 0).mean()), "nfeatures": nfeatures, "npcs": npcs}
    emb, res["embed_wall"] = wall(lambda: preprocess.embed(X, nfeatures=nfeatures, npcs=npcs), reps)
    res["embed_host_parts_s"] = {k: emb.timing[k] for k in ("loess_s", "eigh_s")}
    t0 = time.perf_counter()
    with preprocess.ExpressionMatrix(X) as m:
        res["upload_s"] = time.perf_counter() - t0
        k = {}
        k["normalize"] = median_ms(m, "normalize_ms", lambda: m.normalize(1e4), reps)
        k["gene_stats_counts"] = median_ms(m, "gene_stats_counts_ms", lambda: (m._stats.pop(0, None), m.gene_stats("counts")), reps)
        k["gene_stats_normalized"] = median_ms(m, "gene_stats_normalized_ms",
                                               lambda: (m._stats.pop(1, None), m.gene_stats("normalized")), reps)
        mean, var, _ = m.gene_stats("counts")
        sd = np.sqrt(emb.features.variance_expected)
        k["clipped_variance"] = median_ms(m, "clipped_variance_ms", lambda: m.clipped_variance(mean, sd, np.sqrt(n)), reps)
        k["select"] = median_ms(m, "select_ms", lambda: preprocess._select_scaled(m, emb.genes, 10.0), reps)
        k["gram"] = median_ms(m, "gram_ms", m.gram, reps)
        V = emb.loadings.astype(np.float32)
        k["project"] = median_ms(m, "project_ms", lambda: m.project(V), reps)
        res["kernels"] = k
        res["kernel_sum_median_ms"] = float(sum(v["median_ms"] for v in k.values()))
        res["gram_tf_executed"] = gram_flops(n, nfeatures) / (k["gram"]["median_ms"] * 1e-3) / 1e12
        res["gram_fraction_of_f32_mfma_peak"] = res["gram_tf_executed"] / PEAK_F32_MFMA_TF

    # the same chain on the host, fp64
    h = {}
    t0 = time.perf_counter(); Y = ref.normalize(X); h["normalize_s"] = time.perf_counter() - t0
    t0 = time.perf_counter(); hmean, hvar, _ = ref.gene_stats(X); ymean, yvar, _ = ref.gene_stats(Y); h["gene_stats_s"] = time.perf_counter() - t0
    t0 = time.perf_counter(); hsd = preprocess.expected_sd_from_stats(hmean, hvar); h["loess_s"] = time.perf_counter() - t0
    t0 = time.perf_counter(); vs = ref.clipped_variance(X, hmean, hsd, np.sqrt(n)); h["clipped_variance_s"] = time.perf_counter() - t0
    genes = preprocess.top_features(vs, nfeatures)
    t0 = time.perf_counter()
    Z = np.minimum((Y[:, genes].astype(np.float64) - ymean[genes]) / np.sqrt(yvar[genes]), 10.0)
    h["scale_s"] = time.perf_counter() - t0
    t0 = time.perf_counter(); G = Z.T @ Z; h["gram_s"] = time.perf_counter() - t0
    t0 = time.perf_counter(); r = preprocess.pca_from_gram(G, n, npcs); h["eigh_s"] = time.perf_counter() - t0
    t0 = time.perf_counter(); coords = Z @ r.loadings; h["project_s"] = time.perf_counter() - t0
    h["total_s"] = float(sum(h.values()))
    res["host_fp64"] = h
    res["genes_shared_with_host"] = int(len(set(genes.tolist()) & set(emb.genes.tolist())))
    res["eigenvalues_max_rel_diff_vs_host"] = float(np.max(np.abs(emb.eigenvalues - r.eigenvalues) / r.eigenvalues))
    res["abs_coords_max_diff_vs_host"] = float(np.max(np.abs(np.abs(emb.coords[:, :5]) - np.abs(coords[:, :5]))))
    return res


def products_shape(rng, reps, n, h, p):
    X = counts(rng, n, h)
    res = {"n": n, "features": h, "p": p, "gram_chunk": preprocess.GRAM_CHUNK}
    with preprocess.ExpressionMatrix(X) as m:
        m.normalize()
        preprocess._select_scaled(m, np.arange(h), 10.0)
        res["gram"] = median_ms(m, "gram_ms", m.gram, reps)
        V = rng.normal(size=(h, p)).astype(np.float32)
        res["project"] = median_ms(m, "project_ms", lambda: m.project(V), reps)
        Z = m.fetch_scaled()
    res["gram_tf_executed"] = gram_flops(n, h) / (res["gram"]["median_ms"] * 1e-3) / 1e12
    res["gram_fraction_of_f32_mfma_peak"] = res["gram_tf_executed"] / PEAK_F32_MFMA_TF
    res["project_tf"] = 2.0 * n * h * p / (res["project"]["median_ms"] * 1e-3) / 1e12
    Z64 = Z.astype(np.float64)
    t0 = time.perf_counter(); Z64.T @ Z64; res["host_fp64_gram_s"] = time.perf_counter() - t0
    t0 = time.perf_counter(); Z64 @ V.astype(np.float64); res["host_fp64_project_s"] = time.perf_counter() - t0
    return res


HOST_PARTS_SRC = """
#include "%s"
extern "C" int host_check(const int64_t *indptr, const int32_t *indices, const float *data, int n, int g) {
    char msg[160];
    return mi_prep_csr::check(indptr, indices, data, n, g, 1 << 23, 2147483647ll, msg, sizeof msg);
}
extern "C" long long host_transpose(const int64_t *indptr, const int32_t *indices, int n, int g) {
    std::vector<int64_t> colptr; std::vector<int32_t> rows, pos;
    mi_prep_csr::transpose(indptr, indices, n, g, colptr, rows, pos);
    return (long long)colptr.back() + (rows.empty() ? 0 : rows.back() + pos.back());
}
"""


def host_parts(csr, reps):
    """seconds of the checks and of the transpose of mi_prep_create_csr_f32, on the host alone (median over reps)"""
    header = os.path.join(ROOT, "scrna_seq_qannealing_clustering_amd", "csrc", "mi_prep_csr.h")
    indptr, indices, data, (n, g) = csr
    with tempfile.TemporaryDirectory() as tmp:
        src, so = os.path.join(tmp, "parts.cpp"), os.path.join(tmp, "parts.so")
        with open(src, "w") as f:
            f.write(HOST_PARTS_SRC % header)
        subprocess.check_call(["g++", "-std=c++17", "-O3", "-fPIC", "-shared", "-o", so, src])
        lib = ctypes.CDLL(so)
        lib.host_transpose.restype = ctypes.c_longlong
        a = (indptr.ctypes.data_as(ctypes.c_void_p), indices.ctypes.data_as(ctypes.c_void_p))
        d = data.ctypes.data_as(ctypes.c_void_p)
        _, check_t = wall(lambda: lib.host_check(a[0], a[1], d, n, g), reps)
        _, transpose_t = wall(lambda: lib.host_transpose(a[0], a[1], n, g), reps)
    return {"check": check_t, "transpose": transpose_t}


def passes_ms(handles, reps, genes, V, sd, n):
    """kernel ms of every pass on each handle of `handles` (name -> ExpressionMatrix), alternating between them"""
    calls = {
        "normalize": ("normalize_ms", lambda m: m.normalize(1e4)),
        "gene_stats_counts": ("gene_stats_counts_ms", lambda m: (m._stats.pop(0, None), m.gene_stats("counts"))),
        "gene_stats_normalized": ("gene_stats_normalized_ms", lambda m: (m._stats.pop(1, None), m.gene_stats("normalized"))),
        "clipped_variance": ("clipped_variance_ms", lambda m: m.clipped_variance(m.gene_stats("counts")[0], sd, np.sqrt(n))),
        "select": ("select_ms", lambda m: preprocess._select_scaled(m, genes, 10.0)),
        "gram": ("gram_ms", lambda m: m.gram()),
        "project": ("project_ms", lambda m: m.project(V)),
    }
    out = {name: {} for name in handles}
    for pass_name, (key, call) in calls.items():
        ms = {name: [] for name in handles}
        for rep in range(reps + 1):
            for name, m in handles.items():
                call(m)
                if rep:
                    ms[name].append(m.timing[key])
        for name in handles:
            out[name][pass_name] = {"ms": ms[name], "median_ms": float(np.median(ms[name]))}
    for name in handles:
        out[name]["kernel_sum_median_ms"] = float(sum(v["median_ms"] for v in out[name].values()))
    return out


def sparse_pbmc_shape(rng, reps, nfeatures, npcs):
    import scipy.sparse as sp
    n, g = 2638, 13714
    X = counts(rng, n, g, log_rate=-3.95)
    A = sp.csr_matrix(X)
    res = {"n": n, "genes": g, "nonzero_share": float((X != 0).mean()), "nnz": int(A.nnz), "nfeatures": nfeatures, "npcs": npcs}
    csr = preprocess.canonical_csr(A)
    res["create_host_parts_s"] = host_parts(csr, reps)

    def create(M):
        m = preprocess.ExpressionMatrix(M)
        b = m.device_bytes()
        m.close()
        return b
    res["dense_device_bytes_after_create"], res["dense_create_wall"] = wall(lambda: create(X), reps)
    res["sparse_device_bytes_after_create"], res["sparse_create_wall"] = wall(lambda: create(A), reps)
    emb_d, res["dense_embed_wall"] = wall(lambda: preprocess.embed(X, nfeatures=nfeatures, npcs=npcs), reps)
    emb_s, res["sparse_embed_wall"] = wall(lambda: preprocess.embed(A, nfeatures=nfeatures, npcs=npcs), reps)
    res["embed_identical"] = bool(np.array_equal(emb_d.genes, emb_s.genes) and np.array_equal(emb_d.coords, emb_s.coords)
                                  and np.array_equal(emb_d.eigenvalues, emb_s.eigenvalues))
    sd = np.sqrt(emb_d.features.variance_expected)
    V = emb_d.loadings.astype(np.float32)
    with preprocess.ExpressionMatrix(X) as d, preprocess.ExpressionMatrix(A) as s:
        res["kernels"] = passes_ms({"dense": d, "sparse": s}, reps, emb_d.genes, V, sd, n)
        res["dense_device_bytes"], res["sparse_device_bytes"] = d.device_bytes(), s.device_bytes()
        res["passes_identical"] = bool(
            np.array_equal(d.fetch_normalized(), s.fetch_normalized().toarray())
            and all(np.array_equal(a, b) for w in ("counts", "normalized") for a, b in zip(d.gene_stats(w), s.gene_stats(w)))
            and np.array_equal(d.fetch_scaled(), s.fetch_scaled()) and np.array_equal(d.gram(), s.gram()))
    k = res["kernels"]
    res["sparse_over_dense_kernel_ms"] = {p: k["sparse"][p]["median_ms"] / k["dense"][p]["median_ms"]
                                          for p in k["dense"] if p != "kernel_sum_median_ms"}
    return res


def sparse_beyond_dense(rng, reps, n, g, per_cell, nfeatures, npcs):
    import scipy.sparse as sp
    t0 = time.perf_counter()
    total = n * per_cell
    A = sp.coo_matrix((rng.integers(1, 21, total).astype(np.float32),
                       (np.repeat(np.arange(n, dtype=np.int32), per_cell), rng.integers(0, g, total, dtype=np.int32))),
                      shape=(n, g)).tocsr()
    A.sum_duplicates()
    res = {"n": n, "genes": g, "entries": n * g, "dense_limit_entries": 2 ** 32, "nnz": int(A.nnz),
           "nonzero_share": A.nnz / (n * g), "generate_s": time.perf_counter() - t0, "nfeatures": nfeatures, "npcs": npcs}
    csr = preprocess.canonical_csr(A)
    res["create_host_parts_s"] = host_parts(csr, reps)

    def create():
        preprocess.ExpressionMatrix(A).close()
    _, res["sparse_create_wall"] = wall(create, reps)
    with preprocess.ExpressionMatrix(A) as s:
        res["device_bytes_after_create"] = s.device_bytes()
        s.normalize(1e4)
        mean, var, cnt = s.gene_stats("counts")
        genes = np.argsort(-cnt, kind="stable")[:nfeatures].astype(np.int32)
        V = rng.normal(size=(nfeatures, npcs)).astype(np.float32)
        res["kernels"] = passes_ms({"sparse": s}, reps, genes, V, np.sqrt(var), n)["sparse"]
        res["device_bytes_after_select"] = s.device_bytes()
    res["dense_bytes_per_matrix_would_be"] = 4 * n * g
    return res


def main_sparse(args):
    rng = np.random.default_rng(0)
    out = {"reps": args.reps, "device": _lib.device_info(0), "host_threads_env": os.environ.get("OMP_NUM_THREADS"),
           "host_cpus_usable": len(os.sched_getaffinity(0))}
    out["pbmc3k_shape_6_percent"] = sparse_pbmc_shape(rng, args.reps, args.nfeatures, args.npcs)
    print("pbmc3k_shape_6_percent", json.dumps(out["pbmc3k_shape_6_percent"]), flush=True)
    out["beyond_dense_70000x65536"] = sparse_beyond_dense(rng, args.reps, 70000, 65536, 700, args.nfeatures, args.npcs)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sparse", action="store_true", help="measure the sparse handle against the dense one (see above)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nfeatures", type=int, default=2000)
    ap.add_argument("--npcs", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    if args.sparse:
        out = main_sparse(args)
    else:
        out = {"reps": args.reps, "device": _lib.device_info(0), "peak_f32_mfma_tf": PEAK_F32_MFMA_TF,
               "host_threads_env": os.environ.get("OMP_NUM_THREADS"), "host_cpus_usable": len(os.sched_getaffinity(0))}
        out["pbmc3k_shape"] = pbmc_shape(rng, args.reps, args.nfeatures, args.npcs)
        print("pbmc3k_shape", json.dumps(out["pbmc3k_shape"]), flush=True)
        out["products_50000x2000"] = products_shape(rng, args.reps, 50000, 2000, args.npcs)
    s = json.dumps(out, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
