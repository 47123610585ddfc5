"""Times run_tsne at the three shapes of profiles/tsne.json and writes that file's content to stdout / --out.

    python scripts/perf_tsne.py --out profiles/tsne.json [--no-reference]

Shapes: the PBMC3k shape (n = 2638, 10 PCs, perplexity 30, 1000 iterations), n = 10 000 (the notebook's PBMC10k, 1000
iterations) and n = 50 000 (100 iterations), synthetic Gaussian blobs with Rtsne's defaults otherwise.  Per shape: kernel ms per
stage and per iteration (HIP events), the whole warmed call (host clock; the call ends in device-to-host copies), and the
repulsion kernel alone against its VALU model.  The numpy restatement of one layout iteration (row blocks of the same
all-pairs sums, fp64) is timed on the CPUs of the same machine and SCALED to the iteration count (at n = 50 000 also over
the row blocks: every 8th is run)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from scrna_seq_qannealing_clustering_amd import _lib, metrics, tsne  # noqa: E402

# k_tsne_repulse per pair, counted in the source (c = 2 / 3): c subtractions, 1 multiply + (c - 1) fma for |d|^2, 1 add, the
# compare / select of j = i, 1 add (sum q), 1 multiply (q^2), c fma  -> 11 / 14 full-rate VALU instructions, plus v_rcp_f32 at a
# quarter of the rate (4 issue slots); the ds_read of y_j is not VALU.  A wave64 instruction takes 2 cycles on a SIMD-32.
VALU_SLOTS_PER_PAIR = {2: 11 + 4, 3: 14 + 4}
LANES_PER_CLOCK = 256 * 4 * 32                               # CUs x SIMDs x lanes
CLOCK_HZ = 2.4e9


def blobs(n, dim, groups, seed):
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(groups, dim)) * 6.0
    return (centres[rng.integers(0, groups, n)] + rng.normal(size=(n, dim))).astype(np.float32)


def repulse_alone_ms(Y, repeats=20):
    """k_tsne_repulse alone: the KL divergence of an EMPTY graph launches it and a k_tsne_kl that finds nothing to add; each
    kernel sits between its own pair of events.  Returns (best ms at Y, best ms of the same two launches at n = 2: what
    two event pairs around nothing cost, to be read against the first)."""
    def best(Y):
        rowptr = np.zeros(len(Y) + 1, dtype=np.int64)
        col, P = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32)
        return min(tsne.kl_divergence(rowptr, col, P, Y, return_ms=True)[1] for _ in range(repeats))
    return best(Y), best(np.ascontiguousarray(Y[:2]))


def numpy_iteration_s(rowptr, col, P, Y, every=1, block=512):
    """one layout iteration's sums in numpy fp64, row block by row block (every `every`-th block is run) -> seconds"""
    Y = Y.astype(np.float64)
    n = len(Y)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    t0 = time.perf_counter()
    d = Y[rows] - Y[col]
    pq = P.astype(np.float64) / (1.0 + (d * d).sum(axis=1))
    attr = np.zeros_like(Y)
    for c in range(Y.shape[1]):
        attr[:, c] = np.bincount(rows, weights=pq * d[:, c], minlength=n)
    rep, Z = np.zeros_like(Y), 0.0
    for b, lo in enumerate(range(0, n, block)):
        if b % every:
            continue
        diff = Y[lo:lo + block, None, :] - Y[None, :, :]
        q = 1.0 / (1.0 + (diff * diff).sum(axis=2))
        q[np.arange(len(q)), lo + np.arange(len(q))] = 0.0
        Z += q.sum()
        rep[lo:lo + block] = ((q * q)[:, :, None] * diff).sum(axis=1)
    (12.0 * attr - rep / max(Z, 1.0)).sum()
    return time.perf_counter() - t0


def measure(X, perplexity, T, repeats):
    tsne.run_tsne(X[:512], perplexity=perplexity, n_iter=5)                     # module load, first-launch costs
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = tsne.run_tsne(X, perplexity=perplexity, n_iter=T)
        runs.append(((time.perf_counter() - t0) * 1e3, r))
    again = tsne.run_tsne(X, perplexity=perplexity, n_iter=T)
    wall, r = min(runs, key=lambda x: x[0])
    n, g = len(X), r.graph
    model_ms = n * (n - 1.0) * VALU_SLOTS_PER_PAIR[2] / (LANES_PER_CLOCK * CLOCK_HZ) * 1e3
    rep_ms, two_empty_spans_ms = repulse_alone_ms(r.coords)
    return r, {
        "n": int(n), "dim": int(X.shape[1]), "perplexity": perplexity, "K": int(g.nn.shape[1]), "n_iter": T,
        "chunks_S": tsne.chunks(n), "lanes_G": tsne.lanes(int(g.rowptr[-1]), n),
        "nnz": int(g.rowptr[-1]), "mean_degree": float(g.rowptr[-1] / n), "max_degree": int(g.max_degree),
        "kernel_ms": {s: r.timing[s] for s in ("knn_ms", "calibrate_ms", "symmetrize_ms", "layout_ms", "kl_ms")},
        "ms_per_iteration": r.timing["iter_ms"], "host_ms": r.timing["host_ms"], "end_to_end_wall_ms": wall,
        "end_to_end_wall_ms_all_repeats": [w for w, _ in runs],
        "kl_divergence": r.kl_divergence,
        "knn_preservation_k30": metrics.knn_preservation(np.concatenate([np.arange(n, dtype=np.int32)[:, None], g.nn[:, :29]],
                                                                        axis=1), r.coords),
        "bit_identical_between_runs": bool(np.array_equal(r.coords, again.coords) and r.kl_divergence == again.kl_divergence),
        "repulsion_valu_model": {
            "pairs_per_iteration": n * (n - 1), "valu_issue_slots_per_pair": VALU_SLOTS_PER_PAIR[2],
            "lanes_per_clock": LANES_PER_CLOCK, "clock_hz": CLOCK_HZ, "model_ms_per_iteration": model_ms,
            "k_tsne_repulse_ms": rep_ms, "two_event_pairs_around_trivial_kernels_ms": two_empty_spans_ms,
            "achieved_fraction_of_model": model_ms / rep_ms,
            "model_over_whole_iteration": model_ms / r.timing["iter_ms"],
            "what": "model time over the time of k_tsne_repulse alone at the final coordinates (events around that kernel, "
                    "plus the span of a k_tsne_kl on an empty graph; best of 20); model_over_whole_iteration divides by the "
                    "iteration's launches together",
        },
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--reference-iters", type=int, default=5)
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("perf_tsne.py needs a GPU: no HIP device visible")
    out = {"device": _lib.device_info(0)["name"], "note": "one session; wall times are the best of --repeats runs"}
    X = blobs(2638, 10, 8, 0)
    r, out["pbmc3k_shape"] = measure(X, 30.0, 1000, a.repeats)
    if not a.no_reference:
        import tsne_reference as ref
        t0 = time.perf_counter()
        rowptr, col, P = ref.affinities(X, 30.0)[4:]
        t1 = time.perf_counter()
        ref.layout(rowptr, col, P, tsne.random_init(len(X), 2, 1), 200.0, 12.0, 250, 0.5, 0.8, 250, a.reference_iters)
        t2 = time.perf_counter()
        per_iter = (t2 - t1) / a.reference_iters
        out["pbmc3k_shape"]["numpy_reference"] = {
            "affinities_wall_s": t1 - t0, "layout_iterations_run": a.reference_iters, "layout_wall_s_per_iteration": per_iter,
            "SCALED_wall_s_for_1000_iterations": (t1 - t0) + 1000 * per_iter,
            "how": "numpy fp64, one process; the layout ran %d iterations and is SCALED to 1000" % a.reference_iters,
            "structure_equal": bool(np.array_equal(rowptr, r.graph.rowptr) and np.array_equal(col, r.graph.col)),
        }
    for key, n, T, seed, every in (("n10000", 10000, 1000, 1, 1), ("n50000", 50000, 100, 2, 8)):
        r, out[key] = measure(blobs(n, 10, 10 if n == 10000 else 12, seed), 30.0, T, max(1, a.repeats - 1))
        if not a.no_reference:
            g = r.graph
            sec = numpy_iteration_s(g.rowptr, g.col, g.P, r.coords, every)
            out[key]["numpy_reference"] = {
                "one_iteration_wall_s": sec * every, "row_blocks_run": "every %d-th of 512 rows" % every,
                "SCALED_layout_wall_s_for_%d_iterations" % T: sec * every * T,
                "how": "numpy fp64, one process: ONE iteration's sums on the device's graph and final coordinates, SCALED to the "
                       "iteration count%s; the affinities are not included" % (" and over the row blocks" if every > 1 else ""),
            }
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
