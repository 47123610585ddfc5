"""The pure parts of csrc/mi_midrank.h (keys, tie-run search, the bitonic network's index arithmetic) under
AddressSanitizer and UBSan: a stand-alone host program (tests/host/midrank_main.cpp) runs them against a linear scan and
``std::sort``."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_midrank_header_is_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "midrank_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "host", "midrank_main.cpp")],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok"), run.stdout + run.stderr
    assert int(run.stdout.split()[1]) > 100000, run.stdout
