"""Times run_umap at the two shapes of profiles/umap_layout.json and writes that file's content to stdout / --out.

    python scripts/perf_umap.py --out profiles/umap_layout.json [--no-reference]

Shapes: the PBMC3k shape (n = 2638, 15 PCs, k = 30, T = 500) and n = 50 000 (15 dims, k = 30, T = 200), both synthetic
Gaussian blobs with Seurat's RunUMAP defaults otherwise (cosine).  For the first shape the numpy restatement of the chain
(tests/umap_reference.py) is timed on the CPUs of the same machine: the only baseline there is."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from scrna_seq_qannealing_clustering_amd import _lib, metrics, umap  # noqa: E402


def blobs(n, dim, groups, seed):
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(groups, dim)) * 6.0
    return (centres[rng.integers(0, groups, n)] + rng.normal(size=(n, dim))).astype(np.float32)


def measure(X, k, T, repeats):
    umap.run_umap(X[:512], n_neighbors=k, n_epochs=5)                          # module load, first-launch costs
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = umap.run_umap(X, n_neighbors=k, n_epochs=T)
        wall = (time.perf_counter() - t0) * 1e3
        runs.append((wall, r))
    again = umap.run_umap(X, n_neighbors=k, n_epochs=T)
    wall, r = min(runs, key=lambda x: x[0])
    return r, {
        "n": int(len(X)), "dim": int(X.shape[1]), "n_neighbors": k, "n_epochs": T, "metric": "cosine",
        "nnz": int(r.rowptr[-1]), "mean_degree": float(r.rowptr[-1] / len(X)), "max_degree": int(np.diff(r.rowptr).max()),
        "kernel_ms": {s: r.timing[s] for s in ("knn_ms", "smooth_ms", "union_ms", "layout_ms")},
        "ms_per_epoch": r.timing["epoch_ms"], "host_ms": r.timing["host_ms"], "end_to_end_wall_ms": wall,
        "end_to_end_wall_ms_all_repeats": [w for w, _ in runs],
        "knn_preservation": metrics.knn_preservation(r.nn, r.coords),
        "bit_identical_between_runs": bool(np.array_equal(r.coords, again.coords)),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    out = {"device": _lib.device_info(0)["name"], "note": "one session; wall times are the best of --repeats runs"}
    X = blobs(2638, 15, 8, 0)
    r, out["pbmc3k_shape"] = measure(X, 30, 500, a.repeats)
    if not a.no_reference:
        import umap_reference as ref
        t0 = time.perf_counter()
        nn, rowptr, col, w = ref.reference_graph(X, 30, "cosine")
        t1 = time.perf_counter()
        Y = ref.layout(rowptr, col, w, umap.pca_init(X, 2), r.a, r.b, 1.0, 500, 5, 42)
        t2 = time.perf_counter()
        out["pbmc3k_shape"]["numpy_reference"] = {
            "graph_wall_s": t1 - t0, "layout_wall_s": t2 - t1, "wall_s": t2 - t0,
            "knn_preservation": ref.knn_preservation(nn, Y), "how": "numpy fp64, one process",
            "max_abs_difference_of_final_coordinates": float(np.abs(Y - r.coords).max()),
        }
    _, out["n50000"] = measure(blobs(50000, 15, 12, 1), 30, 200, max(1, a.repeats - 1))
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
