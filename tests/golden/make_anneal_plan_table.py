#!/usr/bin/env python3
"""Record which anneal kernel the library takes for a structured model into tests/golden/anneal_plan_table.json.

THE TABLE IS A RECORDING OF THE LIBRARY AS IT STOOD BEFORE THE PLANNER (csrc/mi_sa_plan.h) EXISTED: it was written on an
MI355X through the public Python API alone (``Problem.csr_rank1`` / ``potts_csr``, ``set_option``, ``kernel_name()``,
``adjacency_bytes_per_slot()``, ``launch_count()``) and is never regenerated from code that plans through that header.
tests/test_anneal_plan.py holds the planner to it without a GPU, tests/test_gpu_anneal_plan.py the library with one.
``cases()``, ``csr_of()`` and ``run_case()`` are imported by both tests, so generator and tests cannot drift apart.

The models are circulant graphs, ``i ~ i +- s`` for consecutive strides ``s = base, base + 1, ...`` (and ``n / 2`` once
where the degree is odd).  Two seats at circular distance >= B never share an aligned block of B seats, so the base decides
the layout the library finds: 1 -> slots with internal edges; 64 -> edge-free 64-seat slots and no wider block (seats i and
i + 64 share a block of 128); 128 -> edge-free blocks of 128, not 256; 256 -> edge-free blocks of 256.  Every run is one
sweep at beta = 1 (two sweeps, a merge phase between them, for the merge rows).

Row-to-branch coverage (branch names as in csrc/mi_sa_plan.h; CU count of the recording: 256)
  model facts   state width half / byte / bit: n = 1024 / 4864 / 9472 (and MI_K2_STATE = byte, bit at 1024)
                D = 16 / 32 / 64 / runtime width: degree 12..16 / 18 / 34 / 66; degree 4098 is the creation error
                pair packing: 624 slots (n = 39936) has it, 625 (n = 40000) and the issue's 159744 / 160000 do not
                16-bit neighbour words: 260 slots (n = 16640) has none; trimmed rows: degree 13, 14, 15 against 12 and 16
                K3f packing: slots without internal edges at D = 16 / 32; Potts n > 40000 is the creation error that
                pre-empts K3f's own LDS limit (n = 81792 / 81920 / 82048)
  plan_csr_rank1
    forced split (k2_split = 1) / forced pair (k2_pair = 1) / both (split wins) / forced on a model without the packing
    auto split: R <= k2_split_max (1024 | 1025, k2_split_max = 0, R - 1, R), one round of cells + 2048 (n = 9472 | 10240
                at R = 1024); k2_split = 2
    auto pair:  R > 1024; pair_run by 8 cells <= 150 KiB (n = 4352) or one round (n = 4864: R = 4096 | 4098); k2_pair = 2
    tw_pair:    one round of at most 8 cus workgroups (R = 4096 | 4098), nearly full rounds (R = 7372 | 7374), the LDS
                of one round (n = 4352: R = 3584 | 3586; n = 4864: R = 1025 | 3584); D = 32 never; k2_tw = 2
    the pair kernel's second thought: more than 64 slots and R > 3584 drops tw (k2_pair = 1 at n = 4352: 3584 | 3586)
    K2p packing: trimmed 16-bit (6144), trimmed 32-bit (6912 / 7424 / 7936), full 16-bit (6400 / 12544), full 32-bit
                (8448 / 16640): degree 12..16 and 18 under k2_trim, k2_nbr16 = 0 / 1 / 2, with and without tw
    choice 2:   weighted -> wide<D, 1, tw>; blocks of 128 / 256 -> wide<16, 2 | 4>, wide<32, 2> with and without tw;
                256 at D = 32 -> split<32, 4>; 64 with tw -> wide<D, 1, tw>, without -> split<D, 1>; k2_wide = 2 ->
                split<D, 1 | 2 | 4>; split's LDS error at 624 slots
    K2:         tw only for R <= 1024 (1024 | 1025), D = 16 / 32 (18 | 34) and byte / bit state (4864, 9472 | 1024)
    weighted:   pair (D = 16, R > 1024, with and without tw), wide (few replicas, tw), else K2 (D = 32 many replicas,
                k2_tw = 2, k2_wide = 2, k2_pair = 2)
  plan_potts    K3f eligible: K = 2, 8 | 9, 16 | 17, 1; D = 16, 32 | 64, 80; slots with internal edges; k3_fast = 2
                KM 8 | 16 (K = 8 | 9); tw for R <= 1024 (1024 | 1025) and k2_tw = 2; node weights on K3f and K3 at every
                width; min_cluster_size 3; merge moves (name suffix, three launches)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

OUT = os.path.join(HERE, "anneal_plan_table.json")
SEED = 20262
BASE = {"in": 1, "b64": 64, "b128": 128, "b256": 256}
MERGE_SUFFIX = " + k_potts_merge"


def circulant(n, layout, degree):
    """CSR (rowptr, col) of the circulant graph on n seats with the given layout and degree (columns sorted per row)."""
    k, half = degree // 2, degree % 2
    strides = np.arange(BASE[layout], BASE[layout] + k, dtype=np.int64)
    assert k == 0 or strides[-1] < n // 2, (n, layout, degree)
    i = np.arange(n, dtype=np.int64)[:, None]
    cols = [(i + strides) % n, (i - strides) % n] + ([(i + n // 2) % n] if half else [])
    col = np.sort(np.concatenate(cols, axis=1), axis=1)
    rowptr = np.arange(n + 1, dtype=np.int64) * degree
    return rowptr.astype(np.int32), col.reshape(-1).astype(np.int32)


def _case(family, n, layout, degree, R, **kw):
    c = {"family": family, "n": n, "layout": layout, "degree": degree, "R": R, "options": {}, "k2_state": None,
         "weighted": False, "K": 2, "node_weights": False, "min_cluster_size": 0, "merge": False}
    for key, v in kw.items():
        if key in c:
            c[key] = v
        else:
            c["options"][key] = v
    tags = ["%s=%s" % (key, c[key]) for key in ("k2_state", "weighted", "K", "node_weights", "min_cluster_size", "merge")
            if kw.get(key)]
    tags += ["%s=%d" % kv for kv in sorted(c["options"].items())]
    c["id"] = "-".join(["%s-n%d-%s-d%d-R%d" % (family, n, layout, degree, R)] + tags)
    return c


def cases():
    """The fixed grid (see the module docstring for what each group covers)."""
    out = []

    def k2(n, layout, degree, R, **kw):
        out.append(_case("k2", n, layout, degree, R, **kw))

    def potts(n, layout, degree, R, K=4, **kw):
        out.append(_case("potts", n, layout, degree, R, K=K, **kw))

    # -- few replicas, every layout and width -----------------------------------------------------------------------------
    for d in (12, 16, 18, 34, 66):
        k2(1024, "in", d, 1)
    for d in (12, 13, 14, 15, 16, 18, 34, 66):
        k2(1024, "b64", d, 1)
    for layout in ("b128", "b256"):
        for d in (12, 18):
            k2(1024, layout, d, 1)
            k2(1024, layout, d, 1, k2_tw=2)
            k2(1024, layout, d, 1, k2_wide=2)
    k2(1024, "b128", 12, 1, k2_wide=1)
    k2(1024, "b128", 12, 1, k2_tw=1)
    k2(1024, "in", 12, 1, k2_tw=2)
    for d in (12, 18):
        k2(1024, "b64", d, 1, k2_tw=2)
        k2(1024, "b64", d, 1, k2_wide=2)
    # -- k2_split / k2_split_max / k2_pair against the default elsewhere ----------------------------------------------------
    k2(1024, "b64", 12, 1, k2_split=2)
    k2(1024, "b64", 12, 2048, k2_split=1)
    k2(1024, "b128", 12, 2048, k2_split=1)
    k2(1024, "in", 12, 1, k2_split=1)
    k2(1024, "b64", 12, 1, k2_split_max=0)
    k2(1024, "b64", 12, 8, k2_split_max=7)
    k2(1024, "b64", 12, 8, k2_split_max=8)
    k2(1024, "b64", 12, 2048, k2_split_max=2048)
    k2(1024, "b64", 12, 1, k2_pair=1)
    k2(1024, "b64", 12, 1, k2_pair=1, k2_split=1)
    k2(1024, "in", 12, 1, k2_pair=1)
    k2(1024, "b64", 12, 2048, k2_pair=2)
    k2(1024, "b64", 12, 2048, k2_pair=2, k2_split=2)
    k2(1024, "in", 12, 2048)
    # -- R thresholds ------------------------------------------------------------------------------------------------------
    for R in (1024, 1025, 3584, 3586, 4096, 4098, 6144, 7372, 7374):
        k2(1024, "b64", 12, R)
    for R in (1, 1024, 1025, 3584, 3586, 4096, 4098):
        k2(4352, "b64", 12, R)
    for R in (3584, 3586, 4096, 4098):
        k2(4352, "b64", 12, R, k2_pair=1)
    k2(4352, "b64", 12, 3586, k2_pair=1, k2_tw=2)
    for R in (1, 1024, 1025, 3584, 4096, 4098):
        k2(4864, "b64", 12, R)
    for R in (1, 1024, 1025):
        k2(9472, "b64", 12, R)
        k2(10240, "b64", 12, R)
    # -- K2p packings: trimmed rows, 16-bit neighbour words ------------------------------------------------------------------
    for d in (12, 13, 14, 15, 16, 18):
        k2(1024, "b64", d, 1025)
        k2(1024, "b64", d, 1025, k2_nbr16=2)
    for d in (13, 15, 16):
        k2(1024, "b64", d, 1025, k2_trim=2)
        k2(1024, "b64", d, 1025, k2_trim=2, k2_nbr16=2)
        k2(1024, "b64", d, 1025, k2_tw=2)
        k2(1024, "b64", d, 4098)
    k2(1024, "b64", 15, 1025, k2_trim=1)
    k2(1024, "b64", 15, 1025, k2_nbr16=1)
    k2(1024, "b64", 15, 1025, k2_tw=1)
    k2(1024, "b64", 34, 1025)
    for d in (12, 15, 18):
        k2(16640, "b64", d, 2, k2_pair=1)
    k2(16640, "b64", 12, 1)
    k2(16640, "b64", 12, 1025)
    # -- the pair-packing limit: 624 | 625 slots; the sizes the issue names lie past it ---------------------------------------
    for n in (39936, 40000, 159744, 160000):
        k2(n, "b64", 12, 1)
        k2(n, "b64", 12, 2, k2_pair=1)
    k2(39936, "b128", 12, 1, k2_split=1, k2_wide=2)
    k2(39936, "b64", 12, 1, k2_wide=2)
    # -- K2 itself: state width x row width x tw ------------------------------------------------------------------------------
    for n in (4864, 9472):
        for d in (12, 18, 34, 66):
            k2(n, "in", d, 1)
        k2(n, "in", 12, 1024)
        k2(n, "in", 12, 1025)
        k2(n, "in", 12, 1, k2_tw=2)
    for state in ("byte", "bit", "half"):
        k2(1024, "in", 12, 1, k2_state=state)
    k2(1024, "b64", 12, 1, k2_state="bit")
    k2(4864, "in", 12, 1, k2_state="bit")
    k2(9472, "in", 12, 1, k2_state="byte")
    k2(8192, "in", 4098, 1)
    # -- pair-term weights -----------------------------------------------------------------------------------------------------
    for R in (1, 2048, 4098):
        k2(1024, "b64", 12, R, weighted=True)
    for R in (1, 2048):
        k2(1024, "b64", 18, R, weighted=True)
    k2(1024, "b64", 12, 1, weighted=True, k2_tw=2)
    k2(1024, "b64", 12, 1, weighted=True, k2_wide=2)
    k2(1024, "b64", 12, 1, weighted=True, k2_pair=1)
    k2(1024, "b64", 12, 2048, weighted=True, k2_pair=2)
    k2(1024, "b64", 12, 2048, weighted=True, k2_tw=2)
    # -- Potts -------------------------------------------------------------------------------------------------------------------
    for K in (1, 2, 8, 9, 16, 17):
        potts(1024, "b64", 12, 1, K=K)
    potts(1024, "b64", 12, 1, K=65)
    for layout in ("b64", "in"):
        for d in (12, 18, 34, 66):
            potts(1024, layout, d, 1)
            potts(1024, layout, d, 1, node_weights=True)
    for R in (1024, 1025):
        potts(1024, "b64", 12, R)
        potts(1024, "b64", 12, R, K=9, node_weights=True)
    potts(1024, "b64", 12, 1, k2_tw=2)
    potts(1024, "b64", 12, 1, k3_fast=2)
    potts(1024, "b64", 12, 1, k3_fast=1)
    potts(1024, "b64", 12, 1, k3_fast=2, node_weights=True)
    for layout in ("b64", "in"):
        potts(1024, layout, 12, 1, min_cluster_size=3)
        potts(1024, layout, 12, 1, merge=True)
        potts(1024, layout, 12, 1, merge=True, node_weights=True)
    potts(1024, "b64", 18, 1025, K=16, min_cluster_size=3)
    for n in (39936, 40000, 81792, 81920, 82048):
        potts(n, "b64", 12, 1)
    unique = list({c["id"]: c for c in out}.values())          # (a shape that two groups name is one row)
    assert len(unique) <= 200, len(unique)
    return unique


def csr_of(case):
    """(rowptr, col, val) of the CALLER's model of a case; a weighted case has two more variables, without couplings."""
    rowptr, col = circulant(case["n"], case["layout"], case["degree"])
    if case["weighted"]:
        rowptr = np.concatenate([rowptr, [rowptr[-1]] * 2]).astype(np.int32)
    val = np.full(len(col), 1.0 if case["family"] == "k2" else -1.0, dtype=np.float32)
    return rowptr, col, val


def pair_weights(case):
    return np.array([1] * case["n"] + [2, 4], dtype=np.int64)


def run_case(case, device=0):
    """Create the problem, set the options, anneal once; what the library reports, or the error of the step that failed."""
    from scrna_seq_qannealing_clustering_amd import _lib
    from scrna_seq_qannealing_clustering_amd.engine import Problem
    rowptr, col, val = csr_of(case)
    c_pair = 0.01
    saved = os.environ.pop("MI_K2_STATE", None)
    if case["k2_state"]:
        os.environ["MI_K2_STATE"] = case["k2_state"]
    prob = None
    try:
        if case["family"] == "k2":
            lin = np.full(len(rowptr) - 1, -1.0, dtype=np.float32)
            if case["weighted"]:
                prob = Problem.csr_rank1(rowptr, col, val, lin, c_pair, device=device, order="padded",
                                         weights=pair_weights(case))
            else:
                prob = Problem.csr_rank1(rowptr, col, val, lin, c_pair, device=device, order=None)
        else:
            n, K = case["n"], case["K"]
            nw = (np.ones(n, dtype=np.int32), np.full(n, c_pair, dtype=np.float32), None) if case["node_weights"] else None
            prob = Problem.potts_csr(rowptr, col, val, c_pair, n, K, device=device, order=None, node_weights=nw)
            if case["min_cluster_size"]:
                prob.set_option("min_cluster_size", case["min_cluster_size"])
            if case["merge"]:
                prob.set_merge_moves(1, None, c_pair if case["node_weights"] else None)
        for key, v in sorted(case["options"].items()):
            prob.set_option(key, v)
        prob.anneal(case["R"], np.ones(2 if case["merge"] else 1), SEED)
        prob.sync()
        rec = {"kernel": prob.kernel_name(), "adjacency_bytes": prob.adjacency_bytes_per_slot(),
               "launches": prob.launch_count()}
        if case["weighted"]:
            rec["n_dev"] = int(prob.n_dev)                  # (the two weighted variables sit in its last slot)
            rec["weighted_slot"] = int(prob.n_dev) // 64 - 1
        return rec
    except _lib.MiSaError as exc:
        return {"error": int(exc.code), "message": exc.message}
    finally:
        if prob is not None:
            prob.close()
        os.environ.pop("MI_K2_STATE", None)
        if saved is not None:
            os.environ["MI_K2_STATE"] = saved


def load_table():
    with open(OUT) as f:
        return json.load(f)


def main():
    from scrna_seq_qannealing_clustering_amd import _lib
    rows = []
    for case in cases():
        row = dict(case)
        row.update(run_case(case))
        rows.append(row)
        print(row["id"], "->", row.get("kernel", row.get("message")), row.get("adjacency_bytes"), row.get("launches"),
              flush=True)
    out = {"compute_units": _lib.device_info(0)["compute_units"], "device": _lib.device_info(0)["name"],
           "recorded_at": sys.argv[1] if len(sys.argv) > 1 else None, "seed": SEED, "rows": rows}
    with open(sys.argv[2] if len(sys.argv) > 2 else OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
