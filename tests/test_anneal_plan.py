"""The host-only planner (csrc/mi_sa_plan.h through mi_sa_plan_anneal) against the recording of what the library chose
before the planner existed (tests/golden/anneal_plan_table.json, written on an MI355X by make_anneal_plan_table.py).
No GPU: every row's CSR is rebuilt, planned with the CU count the table was recorded with, and must give the recorded
kernel name and adjacency byte count, or the recorded error code and message.  No row is skipped."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import make_anneal_plan_table as mk  # noqa: E402
from scrna_seq_qannealing_clustering_amd import _lib, engine  # noqa: E402

TABLE = mk.load_table()
ROWS = TABLE["rows"]


def device_model(row):
    """(kind, rowptr, col, n, weighted slot) of the model as the device sees it."""
    rowptr, col, val = mk.csr_of(row)
    if row["family"] == "potts":
        return _lib.KIND_POTTS_CSR, rowptr, col, row["n"], -1
    if not row["weighted"]:
        return _lib.KIND_CSR_RANK1, rowptr, col, row["n"], -1
    # the layout Problem.csr_rank1(order="padded", weights=...) gives the model, by the engine's own host helper
    lin = np.full(len(rowptr) - 1, -1.0, dtype=np.float32)
    rp, cc, _, _, wdev, _, n_dev, _, _ = engine.weighted_layout_csr(rowptr, col, val, lin, mk.pair_weights(row))
    slots = np.unique(np.flatnonzero(wdev != 1) // 64)
    assert len(slots) == 1
    if "n_dev" in row:
        assert (n_dev, int(slots[0])) == (row["n_dev"], row["weighted_slot"])
    return _lib.KIND_CSR_RANK1, rp, cc, n_dev, int(slots[0])


def test_the_table_is_the_grid():
    """One recorded row per case of the generator's grid, with the case's parameters, and the CU count it was made with."""
    cases = mk.cases()
    assert [r["id"] for r in ROWS] == [c["id"] for c in cases]
    for row, case in zip(ROWS, cases):
        assert {k: row[k] for k in case} == case
        assert ("error" in row) != ("kernel" in row)
    assert TABLE["compute_units"] > 0


@pytest.mark.parametrize("row", ROWS, ids=[r["id"] for r in ROWS])
def test_plan_matches_the_recording(row, monkeypatch):
    monkeypatch.delenv("MI_K2_STATE", raising=False)
    if row["k2_state"]:
        monkeypatch.setenv("MI_K2_STATE", row["k2_state"])
    kind, rowptr, col, n, wslot = device_model(row)
    args = (kind, rowptr, col, n, row["R"], row["K"], TABLE["compute_units"], row["options"], wslot,
            row["node_weights"], row["min_cluster_size"])
    if "error" in row:
        with pytest.raises(_lib.MiSaError) as exc:
            engine.plan_anneal(*args)
        assert (exc.value.code, exc.value.message) == (row["error"], row["message"])
        return
    name, adj_bytes = engine.plan_anneal(*args)
    recorded = row["kernel"]
    if row["merge"]:                       # (the merge phase is no part of the plan: its kernel's name follows the planned one)
        assert recorded.endswith(mk.MERGE_SUFFIX)
        recorded = recorded[:-len(mk.MERGE_SUFFIX)]
    assert (name, adj_bytes) == (recorded, row["adjacency_bytes"])


def test_options_are_spelled_once():
    """The option string takes the keys of mi_sa_set_option and nothing else."""
    rowptr, col = mk.circulant(1024, "b64", 12)
    args = (_lib.KIND_CSR_RANK1, rowptr, col, 1024, 2048)
    assert engine.plan_anneal(*args, options="k2_pair=2,k2_split=2")[0] == engine.plan_anneal(
        *args, options={"k2_pair": 2, "k2_split": 2})[0] == "k_anneal_csr_rank1<16, 2>"
    for bad in ("k2_pear=1", "k2_pair=3", "k2_pair", "k2_pair=1x", "min_cluster_size=3"):
        with pytest.raises(_lib.MiSaError) as exc:
            engine.plan_anneal(*args, options=bad)
        assert exc.value.code == -1 and "unknown option" in exc.value.message
