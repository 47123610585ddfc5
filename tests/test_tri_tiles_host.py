"""The tile decode of the agreement and co-association kernels (csrc/mi_tri_tiles.h: tile number -> (bi, bj) on or above
the diagonal of the block grid) off the GPU.  The kernels and tests/host/tri_tiles_main.cpp compile the same text; the
program compares it with a plain double loop over bi <= bj for every tile of every nb up to 400, and at both ends of every
tile row for nb = 782 (the largest a consensus test launches), 1024, 4096, 16 384 and 65 536 (the most the ABI admits,
q up to 2.1e9), where the fp64 guess is furthest from exact."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LARGE = (782, 1024, 4096, 16384, 65536)


def build(tmp_path):
    exe = str(tmp_path / "tri_tiles")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "host", "tri_tiles_main.cpp")], check=True)
    return exe


def test_decode_equals_the_double_loop(tmp_path):
    exe = build(tmp_path)
    r = subprocess.run([exe, "400"] + [str(nb) for nb in LARGE], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    every = sum(nb * (nb + 1) // 2 for nb in range(1, 401))
    assert r.stdout.split() == ["ok", str(every + sum(2 * nb + 1 for nb in LARGE))]


def test_program_counts_every_tile_and_refuses_nb_above_the_abi(tmp_path):
    """the count it prints for a small sweep is the number of tiles (no q is skipped), and an nb the kernels never see is
    refused, not checked in part"""
    exe = build(tmp_path)
    r = subprocess.run([exe, "7", "5"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["ok", str(sum(nb * (nb + 1) // 2 for nb in range(1, 8)) + 11)]
    assert subprocess.run([exe, "3", "65537"], capture_output=True, text=True).returncode == 2
