"""Batched connected components on the device (mi_graph_components) against the host, both forms of the kernel:
  (a) 4096 reads on the bench graph (n = 2638): every read's clusters split into their connected pieces;
  (b) 256 reads x n = 50 000, the SNN graph of config 4 (scripts/run_configs.py; above the LDS limit: the global form
      either way);
  (c) the consensus path: a keep mask per resolution group (8 groups) on the bench graph's edges against the host
      union-find of metrics.consensus_labels on the same edges.
Reads: a planted labelling with 10 % of the cells relabelled at random (K = 16), so many clusters are disconnected.
Beside each device number the time of the scipy loop over the same items (scipy.sparse.csgraph.connected_components on
the filtered graph; measured on --host-sample items and scaled).  Kernel milliseconds from HIP events and wall
milliseconds of the whole call (upload, kernel, download), median over --reps after a warm-up.  No threshold: the
numbers are recorded.  Prints one JSON document (and writes --out).

    python scripts/perf_components.py --reps 5 --out profiles/components_batched.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components as scipy_components

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from scrna_seq_qannealing_clustering_amd import _lib, graphs, metrics, models, snn  # noqa: E402
from scrna_seq_qannealing_clustering_amd.sampler import model_edges  # noqa: E402


def device_call(rowptr, col, n, L, keep, flags):
    """one mi_graph_components call: (labels, counts, kernel ms, wall ms)"""
    B = len(L) if L is not None else len(keep)
    out = np.empty((B, n), dtype=np.int32)
    cnt = np.empty(B, dtype=np.int32)
    ms = C.c_float(0.0)
    i32p = C.POINTER(C.c_int32)
    ptr = (lambda a, t: None if a is None else a.ctypes.data_as(t))
    t0 = time.perf_counter()
    _lib.check(_lib.load().mi_graph_components(rowptr.ctypes.data_as(i32p), col.ctypes.data_as(i32p), n,
                                               ptr(L, C.POINTER(C.c_uint16)), ptr(keep, C.POINTER(C.c_uint8)), B, 0, flags,
                                               out.ctypes.data_as(i32p), cnt.ctypes.data_as(i32p), C.byref(ms)))
    return out, cnt, float(ms.value), (time.perf_counter() - t0) * 1e3


def timed(rowptr, col, n, L, keep, flags, reps):
    k, w = [], []
    for rep in range(reps + 1):
        out, cnt, kms, wms = device_call(rowptr, col, n, L, keep, flags)
        if rep:
            k.append(kms)
            w.append(wms)
    return out, cnt, {"kernel_ms": k, "kernel_median_ms": float(np.median(k)), "wall_ms": w, "wall_median_ms": float(np.median(w))}


def scipy_loop_s(n, eu, ev, L, keep, sample):
    """seconds per item of the scipy loop, on the first `sample` items; and its labels for them"""
    labs = []
    t0 = time.perf_counter()
    for b in range(sample):
        live = np.ones(len(eu), dtype=bool)
        if L is not None:
            live &= L[b][eu] == L[b][ev]
        if keep is not None:
            live &= keep[b] != 0
        A = coo_matrix((np.ones(int(live.sum()), dtype=np.int8), (eu[live], ev[live])), shape=(n, n))
        labs.append(scipy_components(A, directed=False)[1])
    return (time.perf_counter() - t0) / sample, labs


def same_partition(a, b):
    return len(np.unique(a)) == len(np.unique(b)) == len(np.unique(a.astype(np.int64) * (int(b.max()) + 1) + b))


def noisy_reads(rng, truth, R, K, noise=0.1):
    L = np.tile(truth % K, (R, 1)).astype(np.uint16)
    flip = rng.random(L.shape) < noise
    L[flip] = rng.integers(0, K, int(flip.sum()))
    return np.ascontiguousarray(L)


def case(name, rowptr, col, eu, ev, n, L, keep, reps, sample, forms):
    res = {"n": int(n), "items": int(len(L) if L is not None else len(keep)), "stored_entries": int(len(col))}
    outs = {}
    for form, flags in forms:
        outs[form], cnt, t = timed(rowptr, col, n, L, keep, flags, reps)
        res[form] = t
    per_item, labs = scipy_loop_s(n, eu, ev, L, keep, sample)
    first = outs[forms[0][0]]
    res["forms_agree"] = all(np.array_equal(first, o) for o in outs.values())
    res["agrees_with_scipy_on_sample"] = all(same_partition(first[b], labs[b]) for b in range(sample))
    res["mean_components"] = float(np.mean(cnt))
    res["host_scipy_s_per_item"] = per_item
    res["host_scipy_s_all_items_scaled"] = per_item * res["items"]
    res["host_sample"] = sample
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--big-n", type=int, default=50000)
    ap.add_argument("--big-reads", type=int, default=256)
    ap.add_argument("--host-sample", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    out = {"reps": args.reps, "lds_max_cells": metrics.COMPONENTS_LDS_MAX_CELLS}
    both = (("lds", 0), ("global", 1))

    # (a) the bench graph, every stored coupling (both directions)
    nodes, su, sv, sw, truth = graphs.synthetic_snn(bench.N_CELLS, bench.K_NN, bench.DIM, bench.ORD, bench.N_CLUSTERS, seed=0,
                                                    spread=bench.SPREAD)                  # (bench.build_workload's graph)
    pm = models.build_modularity_potts(graphs.EdgeListGraph(nodes, su, sv, sw), 1.0, 16)
    n = pm.num_variables
    eu, ev = model_edges(pm)
    rowptr, col = np.ascontiguousarray(pm.rowptr, dtype=np.int32), np.ascontiguousarray(pm.col, dtype=np.int32)
    L = noisy_reads(rng, truth, args.reads, 16)
    out["bench_graph_reads"] = case("bench_graph_reads", rowptr, col, eu, ev, n, L, None, args.reps, args.host_sample, both)

    # (c) the consensus path: 8 groups, a keep mask over the edges (stored once), no labels
    rp1, col1, order = metrics._graph_csr((eu, ev), n)
    counts = rng.integers(0, 257, (8, len(eu)))
    keep = np.ascontiguousarray((counts >= 128)[:, order], dtype=np.uint8)
    res = case("consensus_masks", rp1, col1, eu[order], ev[order], n, None, keep, args.reps, 8, both)
    t0 = time.perf_counter()
    host = [metrics.consensus_labels(counts[g], 256, eu, ev, n, 0.5) for g in range(8)]
    res["host_consensus_labels_s_all_groups"] = time.perf_counter() - t0
    res["equals_consensus_labels"] = bool(np.array_equal(
        np.stack(host), metrics.connected_components((eu, ev), n, keep=counts >= 128)[0]))
    out["consensus_masks"] = res

    # (b) config 4's graph: above the LDS limit, so "lds" (no flag) and "global" (flag) are the same kernel
    Rb, nb = args.big_reads, args.big_n
    r2 = np.random.RandomState(1)
    centers = r2.normal(scale=4.0, size=(30, 15))
    lab = r2.randint(0, 30, size=nb)
    X = (centers[lab] + r2.normal(size=(nb, 15))).astype(np.float32)
    g = snn.build_snn(X, 5, 0.0, 15)
    rowptr = np.ascontiguousarray(g.rowptr, dtype=np.int32)
    col = np.ascontiguousarray(g.col, dtype=np.int32)
    rows = np.repeat(np.arange(nb, dtype=np.int32), np.diff(rowptr))
    L = noisy_reads(rng, lab, Rb, 16)
    out["config4_graph_reads"] = case("config4_graph_reads", rowptr, col, rows, col, nb, L, None, args.reps,
                                      min(args.host_sample, 4), (("global", 1),))
    out["host_threads"] = 1
    s = json.dumps(out, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
