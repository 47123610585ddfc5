"""The work split of the MFMA energy kernel (csrc/mi_energy_plan.h: pieces per state tile from the CU count, the block range
of a piece, the (I, K) walk over the upper block triangle) off the GPU.  The launcher, the kernel and
tests/host/energy_plan_main.cpp compile the same text.  The program sweeps T = 1..48 block rows, 1..64 state tiles and five
CU counts: 1 <= pieces <= S, the ranges tile [0, S) in order, and the kernel's walk from s0 visits exactly the blocks
s0 .. s1 - 1 of the row-major triangle.  Its printed plans pin the Python mirror tests/energy_cases.py:plan, from which the
GPU cases certify the launch they get."""
import os
import subprocess

import pytest

import energy_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = (64, 104, 128, 256, 304)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("energy_plan") / "energy_plan")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-o", out,
                    os.path.join(ROOT, "tests", "host", "energy_plan_main.cpp")], check=True)
    return out


def test_every_plan_tiles_the_triangle_and_the_walk_visits_its_blocks(exe):
    r = subprocess.run([exe, "sweep"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    plans = len(CUS) * 48 * 64
    # every block of every plan is walked once: S blocks per plan, whatever the pieces
    walked = len(CUS) * 64 * sum(T * (T + 1) // 2 for T in range(1, 49))
    assert r.stdout.split() == ["ok", str(plans), str(walked)]


def test_program_refuses_a_malformed_command_line(exe):
    for args in ([], ["plan"], ["plan", "300", "70"], ["plan", "300", "70", "0"], ["sweep", "1"], ["walk"]):
        assert subprocess.run([exe] + args, capture_output=True, text=True).returncode == 2, args


def test_python_mirror_equals_the_printed_plans(exe):
    """the case list at every CU count of the sweep, and a grid of further shapes (n to 48 block rows, R to 64 state tiles)"""
    shapes = [(n, R) for _, n, R in ec.CASES] + [ec.ISOLATION, (130, 3), (257, 100), (1000, 130), (2638, 4096), (300, 300)]
    shapes += [(128 * T - d, 128 * rt - e) for T in (1, 2, 3, 7, 20, 48) for rt in (1, 2, 5, 33, 64) for d, e in ((0, 0), (127, 1))]
    triples = [(n, R, cus) for n, R in shapes for cus in CUS]
    r = subprocess.run([exe, "plan"] + [str(v) for t in triples for v in t], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [tuple(int(v) for v in ln.split()) for ln in r.stdout.splitlines()]
    assert len(lines) == len(triples)
    for (n, R, cus), got in zip(triples, lines):
        p = ec.plan(n, R, cus)
        lens = [s1 - s0 for s0, s1 in p.ranges]
        assert got == (n, R, cus, p.T, p.rtiles, p.S, p.pieces, min(lens), max(lens)), (n, R, cus)
        assert p.U == p.pieces * p.rtiles and p.ranges[0][0] == 0 and p.ranges[-1][1] == p.S
