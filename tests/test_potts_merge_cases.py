"""The edge cases of the merge phase (tests/potts_merge_cases.py) on the restatement alone: every case really merges, and
merges where it is meant to reach -- proposals of the second and third pass of 64, labels held by lanes 32 .. 63, clusters
that are empty from the start, the one merge K = 2 allows, products W_a W_b past 2^53.  Without these a device that never
merged, or never got there, would pass tests/test_gpu_potts_merge_edges.py."""
import collections

import numpy as np
import pytest

import potts_merge_cases as pc
from test_potts_merge_model import chain2e
from scrna_seq_qannealing_clustering_amd import models


def kinds(ref, kind):
    return [t for t in ref.trace if t[0] == kind]


def phases(ref):
    """(replica, sweep) -> that merge phase's trace entries, in proposal order"""
    out = collections.OrderedDict()
    for t in ref.trace:
        out.setdefault((t[1], t[2]), []).append(t)
    return out


@pytest.mark.parametrize("run", pc.RUNS, ids=pc.run_id)
def test_case_reaches_its_path(run):
    name, g, st = run
    c = pc.BY_NAME[name]
    ref = pc.reference(run)
    rp, cc, vv, dq, dc, cq, absent, seats = ref.inputs
    n = len(seats)
    acc, empty = kinds(ref, "accept"), kinds(ref, "empty")
    print("%s: %.2f s, %d merges, %d single-site moves, %d empty skips" % (pc.run_id(run), ref.seconds, ref.merges,
                                                                          ref.accepted, len(empty)))
    # the trace is the whole run: one entry per proposal of every merge phase, the accepted ones the merges
    cuts = [s for s in range(c.sweep_offset, c.sweep_offset + c.S) if s > 0 and s % c.M == 0]
    assert len(ref.trace) == c.R * len(cuts) * c.P and len(acc) == ref.merges
    assert all(len(ph) == c.P and [t[3] for t in ph] == list(range(c.P)) for ph in phases(ref).values())
    assert ref.merges > 0
    assert ref.accepted > 0 or name == "no_couplings"
    two = st == "two"                        # two clusters: one merge per replica at the most, of labels 5 and 63
    if c.P > 64:
        assert any(t[3] >= 64 for t in acc)
    if c.P > 128:
        assert any(t[3] >= 128 for t in acc)
    if c.K >= 33:
        assert any(max(t[4], t[5]) >= 32 for t in acc)
    if c.K >= 34 and not two:                # (K = 33 has one label past 31: no pair of them)
        assert any(min(t[4], t[5]) >= 32 for t in acc)
    if name == "k_above_n" or two:
        assert empty and acc
    if name == "k_above_n":
        assert n < c.K and all(ph[0][0] == "empty" or ph[1][0] == "empty" or ph[2][0] == "empty"
                               for ph in phases(ref).values())
    if two:
        assert all({t[4], t[5]} == {5, 63} for t in acc) and {(t[4], t[5]) for t in acc} == {(5, 63), (63, 5)}
    if c.K == 2:
        # one merge is all a phase can accept; every proposal after it meets an empty cluster
        followed = 0
        for ph in phases(ref).values():
            k = [t[0] for t in ph]
            if "accept" in k:
                at = k.index("accept")
                assert k[at + 1:] == ["empty"] * (c.P - 1 - at) and "empty" not in k[:at]
                followed += at < c.P - 1
            else:                            # (all empty: the sweeps since the last merge left one label unused)
                assert k == ["reject"] * c.P or k == ["empty"] * c.P
        assert followed > 0
    if name in pc.DEVICE_N:
        assert len(rp) - 1 == pc.DEVICE_N[name]
        if name.startswith("ragged"):
            assert not absent.any()
    if name == "opens_two_labels_k64":
        assert len({t[1] for t in acc}) > c.R // 2                        # most replicas merge their two clusters
    if name == "p_64":
        assert any(t[3] == 63 for t in acc)                   # the last lane of the only pass
    if name == "p_65":
        assert any(t[3] == 64 for t in acc)                   # the only lane of the second pass
    if name == "no_couplings":
        assert len(vv) == 0 and models.merge_fixed_exponent(vv) == 0
    if name.startswith("wide_rows"):
        assert int(np.diff(rp).max()) == 129
    if name == "holes":
        assert absent.any() and absent[:int(seats.max())].any()          # holes between the cells, not only behind them
    if c.kind == "heavy":
        assert int(dq.sum()) == pc.WEIGHT_LIMIT
        big = [t[6] for t in ref.trace if t[0] != "empty" and t[6] > 2 ** 53]
        assert big and any(int(float(ww)) != ww for ww in big)           # ... and fp64 does not hold it
    if c.per_replica:
        assert len(set(pc.betas(c, pc.model(name))[1])) == c.R


def test_lanes_and_passes_are_all_reached():
    """Over the table: an accepted proposal in every lane 0 .. 63 of the first pass, and accepted merges into and out of
    every label 0 .. 63."""
    lanes, into, out = set(), set(), set()
    for run in pc.RUNS:
        for t in kinds(pc.reference(run), "accept"):
            lanes.add(t[3] % 64)
            into.add(t[4])
            out.add(t[5])
    assert lanes == set(range(64)) and into == set(range(64)) and out == set(range(64))


def test_trace_leaves_the_run_unchanged():
    run = ("p_65", 0, None)
    c, ref = pc.BY_NAME[run[0]], pc.reference(run)
    rp, cc, vv, dq, dc, cq, absent, seats = ref.inputs
    sched, _ = pc.betas(c, pc.model(c.name))
    lab, acc, merges = chain2e(rp, cc, vv, dq, dc, cq, c.K, c.R, sched, c.seed, c.M, c.P,
                               replica_offset=c.replica_offset, absent=absent)
    assert np.array_equal(lab, ref.labels) and acc == ref.accepted and merges == ref.merges
