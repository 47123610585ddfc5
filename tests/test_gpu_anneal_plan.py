"""The library against the recording of what it chose before the planner existed (tests/golden/anneal_plan_table.json):
every row of the grid is run again -- one sweep -- and must report the recorded kernel name, adjacency byte count and
launch count, or fail with the recorded code and message.  Grouped by family and model size, a few seconds each."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import make_anneal_plan_table as mk  # noqa: E402
from scrna_seq_qannealing_clustering_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

TABLE = mk.load_table()
GROUPS = {}
for _row in TABLE["rows"]:
    GROUPS.setdefault("%s-n%d" % (_row["family"], _row["n"]), []).append(_row)
RECORDED = ("kernel", "adjacency_bytes", "launches", "n_dev", "weighted_slot", "error", "message")


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_library_matches_the_recording(group):
    assert _lib.device_info(0)["compute_units"] == TABLE["compute_units"], "the table's R thresholds are this CU count's"
    wrong = []
    for row in GROUPS[group]:
        got = mk.run_case(row)
        want = {k: row[k] for k in RECORDED if k in row}
        if got != want:
            wrong.append((row["id"], got, want))
    assert not wrong, wrong
