"""Times chain Q (umap.transform, mapping.transfer_labels) at the shapes of profiles/mapping.json and writes that file's content
to stdout / --out.

    python scripts/perf_mapping.py --out profiles/mapping.json [--no-reference]

Shapes (dim = 15, k = 30, c = 2, cosine, synthetic Gaussian blobs): the PBMC3k split (1000 reference cells, 1638 queries,
T = 166), a 50 000-cell split (25 000 / 25 000, T = 66) and the lone-wavefront case (50 000 reference cells, 64 queries: one
workgroup of k_knn_cross streams the whole reference).  Device events per stage plus the wall time of the whole call, warmed,
best of --repeats.  For context: run_umap's per-epoch layout time on the reference set, and for the first shape the numpy
restatement (tests/mapping_reference.py) on the CPUs of the same machine."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from scrna_seq_qannealing_clustering_amd import _lib, mapping, umap  # noqa: E402

K, DIM = 30, 15


def blobs(n, groups, seed):
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(groups, DIM)) * 6.0
    which = rng.integers(0, groups, n)
    return (centres[which] + rng.normal(size=(n, DIM))).astype(np.float32), which


def measure(n_ref, m, T, fit_epochs, repeats, seed):
    X, which = blobs(n_ref + m, 10, seed)
    R, Q, lab = X[:n_ref], X[n_ref:], which[:n_ref]
    fit = umap.run_umap(R, n_neighbors=K, n_epochs=fit_epochs)
    umap.transform(Q[:64], R[:512], umap.UmapResult(fit, coords=fit.coords[:512]), n_neighbors=K, n_epochs=5)   # first-launch costs
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        t = umap.transform(Q, R, fit, n_neighbors=K, n_epochs=T)
        runs.append(((time.perf_counter() - t0) * 1e3, t))
    wall, t = min(runs, key=lambda x: x[0])
    votes = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        v = mapping.transfer_labels(Q, R, lab, k=K, metric="cosine")
        votes.append(((time.perf_counter() - t0) * 1e3, v))
    vwall, v = min(votes, key=lambda x: x[0])
    d2 = ((t.coords[:500, None, :].astype(np.float64) - fit.coords[None].astype(np.float64)) ** 2).sum(axis=2)
    return (R, Q, fit, t), {
        "n_ref": n_ref, "m": m, "dim": DIM, "n_neighbors": K, "n_epochs": T, "metric": "cosine",
        "transform_kernel_ms": {s: t.timing[s] for s in ("knn_ms", "smooth_ms", "init_ms", "layout_ms")},
        "transform_layout_us_per_epoch": 1e3 * t.timing["layout_ms"] / T,
        "transform_host_ms": t.timing["host_ms"], "transform_wall_ms": wall,
        "transform_wall_ms_all_repeats": [w for w, _ in runs],
        "transfer_labels_kernel_ms": dict(v.timing), "transfer_labels_wall_ms": vwall,
        "label_agreement_with_planted": float((v.labels == which[n_ref:]).mean()),
        "nearest_embedded_reference_carries_the_label": float((lab[d2.argmin(axis=1)] == which[n_ref:][:500]).mean()),
        "bit_identical_between_runs": bool(np.array_equal(runs[0][1].coords, runs[-1][1].coords)) if repeats > 1 else None,
        "run_umap_on_the_reference": {"n": n_ref, "n_epochs": fit_epochs, "layout_ms": fit.timing["layout_ms"],
                                      "us_per_epoch": 1e3 * fit.timing["epoch_ms"]},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    out = {"device": _lib.device_info(0)["name"],
           "note": "one session; device events per stage, wall times are the best of --repeats warmed calls"}
    (R, Q, fit, t), out["pbmc3k_split"] = measure(1000, 1638, 166, 500, a.repeats, 0)
    if not a.no_reference:
        import mapping_reference as mref
        t0 = time.perf_counter()
        r = mref.transform(Q, R, fit.coords, K, "cosine", fit.a, fit.b, 0.25, 166, 5, 42)
        out["pbmc3k_split"]["numpy_restatement"] = {
            "wall_s": time.perf_counter() - t0, "how": "numpy fp64, one process",
            "same_neighbours": float((r["nn"] == t.nn).mean()),
            "max_abs_difference_of_final_coordinates": float(np.abs(r["coords"] - t.coords).max())}
    _, out["n50000_split"] = measure(25000, 25000, 66, 200, a.repeats, 1)
    _, out["lone_wavefront"] = measure(50000, 64, 66, 200, a.repeats, 2)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
