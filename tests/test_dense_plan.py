"""The host-only dense planner (csrc/mi_dense_plan.h through mi_sa_plan_dense) against the recording of what the library
chose before the planner existed (tests/golden/dense_plan_table.json, written on an MI355X by make_dense_plan_table.py).
No GPU: every row is planned with the CU count the table was recorded with and must give the recorded kernel name and
launch count, or the recorded error code and message.  No row is skipped."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import make_dense_plan_table as mk  # noqa: E402
from scrna_seq_qannealing_clustering_amd import _lib, engine  # noqa: E402

TABLE = mk.load_table()
ROWS = TABLE["rows"]
# every key of mi_sa_set_option that the dense planner reads, with a value it takes and one it refuses
DENSE_KEYS = {"pace": (0, None), "variant": (4, 5), "unit_rows": (4, 3), "ondemand_permille": (1000, 1001),
              "chunk_sweeps": (0, -1), "mfma_permille": (0, 1001)}


def plan(row, **over):
    # (the table has no row above K1's occupancy: one launch of that kernel holds the row's replicas)
    kw = dict(resync_interval=row["resync"], per_replica=row["per_replica"], cus=TABLE["compute_units"],
              resident_waves=max(4, row["R"]), options=row["options"])
    kw.update(over)
    return engine.plan_dense(row["n"], row["R"], row["sweeps"], **kw)


def test_the_table_is_the_grid():
    """One recorded row per case of the generator's grid, with the case's parameters, and the CU count it was made with."""
    cases = mk.cases()
    assert [r["id"] for r in ROWS] == [c["id"] for c in cases]
    for row, case in zip(ROWS, cases):
        assert {k: row[k] for k in case} == case
        assert ("error" in row) != ("kernel" in row)
    assert TABLE["compute_units"] > 0
    assert {r["n"] for r in ROWS} == {64, 2817, 3521, 4096}


@pytest.mark.parametrize("row", ROWS, ids=[r["id"] for r in ROWS])
def test_plan_matches_the_recording(row):
    if "error" in row:
        with pytest.raises(_lib.MiSaError) as exc:
            plan(row)
        assert (exc.value.code, exc.value.message) == (row["error"], row["message"])
        return
    name, launches, field_bytes = plan(row)
    assert (name, launches) == (row["kernel"], row["launches"])
    # cached fields exactly where the run passes them from launch to launch: [R][64 * NT] floats
    cut = launches > 1 and not name.startswith("k_anneal_dense<")
    nt = 4 * ((row["n"] + 255) // 256)
    assert field_bytes == (row["R"] * nt * 64 * 4 if cut else 0)


def test_a_plan_does_not_depend_on_the_device_where_it_reads_none():
    """K1's occupancy is read only where K1 serves the run: an occupancy of 0 is that kernel's error alone."""
    for row in ROWS:
        if "error" in row:
            continue
        if row["kernel"].startswith("k_anneal_dense<"):
            with pytest.raises(_lib.MiSaError) as exc:
                plan(row, resident_waves=0)
            assert (exc.value.code, exc.value.message) == (-3, "anneal kernel cannot be resident (occupancy 0)")
        else:
            assert plan(row, resident_waves=0) == plan(row)


def test_replicas_above_the_occupancy_take_more_launches():
    assert engine.plan_dense(64, 1000, 3, resident_waves=256, options="variant=1")[:2] == ("k_anneal_dense<4>", 4)
    assert engine.plan_dense(64, 1025, 3, resident_waves=256, options="variant=1")[1] == 5
    assert engine.plan_dense(64, 100000, 3, resident_waves=256, options="variant=1")[1] == 64      # 64 launches at the most


def test_the_large_model_kernels_are_not_planned_here():
    with pytest.raises(_lib.MiSaError) as exc:
        engine.plan_dense(4097, 3, 2)
    assert (exc.value.code, exc.value.message) == (-5, "dense register kernels support n <= 4096 (got 4097)")


def test_options_are_spelled_once():
    """The option string takes the dense keys of mi_sa_set_option, with the values it takes, and nothing else."""
    args = (64, 40, 5)
    assert engine.plan_dense(*args, options="chunk_sweeps=2,variant=2") == engine.plan_dense(
        *args, options={"chunk_sweeps": 2, "variant": 2}) == ("k_anneal_dense_wg<4,4>", 3, 40 * 4 * 64 * 4)
    assert _dense_keys_of_the_header() == set(DENSE_KEYS)
    for key, (good, bad) in DENSE_KEYS.items():
        engine.plan_dense(*args, options="%s=%d" % (key, good))
        if bad is not None:
            with pytest.raises(_lib.MiSaError) as exc:
                engine.plan_dense(*args, options="%s=%d" % (key, bad))
            assert exc.value.code == -1 and exc.value.message == "unknown option '%s'" % key
    for bad in ("varient=1", "variant", "variant=1x", "xl_batched=1", "xl_async=1", "debug=1", "k2_pair=1", "min_cluster_size=3"):
        with pytest.raises(_lib.MiSaError) as exc:
            engine.plan_dense(*args, options=bad)
        assert exc.value.code == -1 and "unknown option" in exc.value.message


def _dense_keys_of_the_header():
    """The keys of kDensePlanOptionKeys, read from the header's text (the table both entry points go through)."""
    import re
    path = os.path.join(os.path.dirname(_lib.__file__), "csrc", "mi_dense_plan.h")
    with open(path) as f:
        text = f.read()
    table = text[text.index("kDensePlanOptionKeys[] = {"):]
    table = table[:table.index("};")]
    return set(re.findall(r'\{"(\w+)", &DensePlanOptions::', table))
