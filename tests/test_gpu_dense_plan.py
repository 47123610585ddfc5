"""The library against the recording of what it chose for dense models of up to 4096 variables before the dense planner existed
(tests/golden/dense_plan_table.json): every row of the grid is run again -- a fresh handle, 0 to 5 sweeps, or 32 | 33 -- and
must report the recorded kernel name and launch count, or fail with the recorded code and message.  Grouped by model size,
so that a group builds its matrix once, in parts of at most 24 rows: a few seconds each."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import make_dense_plan_table as mk  # noqa: E402
from scrna_seq_qannealing_clustering_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

TABLE = mk.load_table()
PART = 24
GROUPS = {}
for _row in TABLE["rows"]:
    _rows = GROUPS.setdefault(mk.group_of(_row), [])
    _rows.append(_row)
PARTS = {"%s-%d" % (g, k // PART): rows[k:k + PART] for g, rows in GROUPS.items() for k in range(0, len(rows), PART)}
RECORDED = ("kernel", "launches", "error", "message")


def test_every_row_is_in_a_part():
    assert sum(len(rows) for rows in PARTS.values()) == len(TABLE["rows"])


@pytest.mark.parametrize("part", sorted(PARTS))
def test_library_matches_the_recording(part):
    assert _lib.device_info(0)["compute_units"] == TABLE["compute_units"], "the table's pacing and occupancy are this CU count's"
    wrong = []
    for row in PARTS[part]:
        got = mk.run_case(row)
        want = {k: row[k] for k in RECORDED if k in row}
        if got != want:
            wrong.append((row["id"], got, want))
    assert not wrong, wrong
