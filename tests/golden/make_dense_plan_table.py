#!/usr/bin/env python3
"""Record which kernel(s) the library takes for a dense model of up to 4096 variables, and in how many launches, into
tests/golden/dense_plan_table.json.

THE TABLE IS A RECORDING OF THE LIBRARY AS IT STOOD BEFORE THE DENSE PLANNER (csrc/mi_dense_plan.h) EXISTED: it was written
on an MI355X through the public Python API alone (``Problem.dense``, ``set_option``, ``anneal``, ``kernel_name()``,
``launch_count()``, or the ``MiSaError`` code and message), a fresh handle per row, and is never regenerated from code that
plans through that header.  tests/test_dense_plan.py holds the planner to it without a GPU, tests/test_gpu_dense_plan.py
the library with one.  ``cases()``, ``model()`` and ``run_case()`` are imported by both tests, so generator and tests
cannot drift apart.

Every run is 0 to 5 sweeps at beta = 1, or 32 | 33 where the default ``chunk_sweeps = 32`` is the subject; the one row
with 4087 sweeps is refused before anything is launched.  The model is the same cheap band matrix at every size: which
kernel serves a run does not depend on the couplings.  Rows are grouped by n (``group_of()``).  (The recording also held
rows for models above 4096 variables; they were taken out with the planner of the large-model kernels, unchanged otherwise.)

Row-to-branch coverage (CU count of the recording: the table's ``compute_units``)
  n <= 4096     models n = 64 / 2817 / 3521 / 4096: NT = 4 (the smallest width) / 48 (the first without K1m) / 56 (the
                first without a 4-row ring) / 64 (the widest)
    variant     0 .. 4 at 19 and 40 replicas; forced 3 above NT = 44 and scheduled (4) at NT >= 48 with >= 32 replicas are
                the K1m refusal; forced 4 that is not cut into launches is K1w
    auto        R = 1, 31 | 32, 127 | 128, 1024 | 1025, in one launch and cut into launches (K1, K1w, scheduled K1m + K1w)
    chunks      chunk_sweeps = 0 / 2 / 32 (the default) with num_sweeps 2 | 3, 5 and 32 | 33; fewer than 32 replicas are never
                cut on a fresh handle; the scheduled form's short first launch (8 sweeps: 33 sweeps are 2 launches)
    unit_rows   0 / 2 / 4, forced K1w and the library's own choice; 4 rows from NT = 56 are the ring refusal
    others      mfma_permille = 0 (auto stays K1w; forced 4 stays scheduled), num_sweeps = 0 (auto is K1), pace = 0,
                one temperature per replica, resync_interval = 2, "too many chunks for the scheduler" (before K1m's refusal)
"""
import functools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

OUT = os.path.join(HERE, "dense_plan_table.json")
SEED = 20263
SMALL = (64, 2817, 3521, 4096)


def _case(n, R, sweeps, per_replica=False, resync=0, **options):
    c = {"n": n, "R": R, "sweeps": sweeps, "per_replica": per_replica, "resync": resync, "options": dict(options)}
    tags = (["per_replica"] if per_replica else []) + (["resync=%d" % resync] if resync else [])
    tags += ["%s=%d" % kv for kv in sorted(options.items())]
    c["id"] = "-".join(["n%d-R%d-s%d" % (n, R, sweeps)] + tags)
    return c


def cases():
    """The fixed grid (see the module docstring for what each group covers)."""
    out = []

    def d(*a, **kw):
        out.append(_case(*a, **kw))

    for n in SMALL:
        # -- every variant, in one launch and cut into launches of 2 sweeps ---------------------------------------------------
        for variant in range(5):
            for R in (19, 40):
                d(n, R, 5, variant=variant)
                d(n, R, 5, variant=variant, chunk_sweeps=2)
            d(n, 40, 5, variant=variant, chunk_sweeps=0)
        for variant in (0, 1, 2):
            d(n, 40, 0, variant=variant)
        for variant in (2, 3, 4):
            for sweeps in (2, 3):
                d(n, 40, sweeps, variant=variant, chunk_sweeps=2)
        # -- the default chunk_sweeps = 32 -------------------------------------------------------------------------------------
        for sweeps in (32, 33):
            d(n, 40, sweeps)
            d(n, 31, sweeps)
            d(n, 40, sweeps, variant=2)
        # -- the library's own variant at its replica thresholds -----------------------------------------------------------------
        for R in (1, 31, 32, 127, 128, 1024, 1025):
            d(n, R, 3)
            d(n, R, 3, chunk_sweeps=2)
        # -- ring unit ---------------------------------------------------------------------------------------------------------
        for unit_rows in (0, 2, 4):
            d(n, 19, 2, variant=2, unit_rows=unit_rows)
            d(n, 40, 5, unit_rows=unit_rows, chunk_sweeps=2)
        d(n, 40, 5, variant=4, unit_rows=4, chunk_sweeps=2)
        # -- the rest --------------------------------------------------------------------------------------------------------------
        d(n, 40, 5, chunk_sweeps=2, mfma_permille=0)
        d(n, 40, 5, variant=4, chunk_sweeps=2, mfma_permille=0)
        d(n, 19, 2, variant=1, pace=0)
        d(n, 19, 2, variant=2, pace=0)
        d(n, 40, 5, per_replica=True, chunk_sweeps=2)
        d(n, 40, 5, per_replica=True, variant=1)
        d(n, 40, 5, resync=2, chunk_sweeps=2)
        d(n, 19, 5, resync=2, variant=3)
    for n in (64, 2817):
        d(n, 40, 4087, variant=4, chunk_sweeps=1)
    unique = list({c["id"]: c for c in out}.values())          # (a shape that two groups name is one row)
    return unique


def group_of(case):
    return "n%d" % case["n"]


@functools.lru_cache(maxsize=1)
def model(n):
    """Qs: ones on the diagonal, -0.25 between neighbours i, i + 1 (fp32, symmetric)."""
    Qs = np.zeros((n, n), dtype=np.float32)
    i = np.arange(n)
    Qs[i, i] = 1.0
    Qs[i[:-1], i[1:]] = Qs[i[1:], i[:-1]] = -0.25
    Qs.setflags(write=False)
    return Qs


def run_case(case, device=0):
    """A fresh handle on the group's model, the options, one anneal; what the library reports, or the error of the step
    that failed."""
    from scrna_seq_qannealing_clustering_amd import _lib
    from scrna_seq_qannealing_clustering_amd.engine import Problem
    prob = None
    try:
        prob = Problem.dense(model(case["n"]), device=device)
        for key, v in sorted(case["options"].items()):
            prob.set_option(key, v)
        if case["per_replica"]:
            prob.anneal(case["R"], np.ones(case["R"]), SEED, resync_interval=case["resync"], num_sweeps=case["sweeps"])
        else:
            prob.anneal(case["R"], np.ones(case["sweeps"]), SEED, resync_interval=case["resync"])
        prob.sync()
        return {"kernel": prob.kernel_name(), "launches": prob.launch_count()}
    except _lib.MiSaError as exc:
        return {"error": int(exc.code), "message": exc.message}
    finally:
        if prob is not None:
            prob.close()


def load_table():
    with open(OUT) as f:
        return json.load(f)


def main():
    import time
    from scrna_seq_qannealing_clustering_amd import _lib
    rows, seconds = [], {}
    for case in cases():
        t0 = time.time()
        row = dict(case)
        row.update(run_case(case))
        rows.append(row)
        seconds[group_of(case)] = seconds.get(group_of(case), 0.0) + time.time() - t0
        print(row["id"], "->", row.get("kernel", row.get("message")), row.get("launches"), flush=True)
    print("seconds per group:", {k: round(v, 1) for k, v in seconds.items()}, flush=True)
    out = {"compute_units": _lib.device_info(0)["compute_units"], "device": _lib.device_info(0)["name"],
           "recorded_at": sys.argv[1] if len(sys.argv) > 1 else None, "seed": SEED, "rows": rows}
    with open(sys.argv[2] if len(sys.argv) > 2 else OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
