"""The engine's HIP-free headers (csrc/mi_sa_plan.h, csrc/mi_sa_pack.h) under AddressSanitizer and UBSan: a stand-alone
host program (tests/host/plan_pack_main.cpp) runs the model facts, the planners and the packers at their edge shapes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planner_and_packers_are_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "plan_pack_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "host", "plan_pack_main.cpp")],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok"), run.stdout + run.stderr
