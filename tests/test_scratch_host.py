"""The owners of csrc/mi_sa_host.h (a call's device scratch, events and stream; a handle's device arrays) and its device
check under AddressSanitizer and UBSan: a stand-alone host program (tests/host/scratch_main.cpp) brings its own fake HIP
runtime, fails every runtime call of a library-shaped entry and of a handle's life in turn, and checks that each way out
frees everything once and that an owner whose allocation failed is empty."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hip_include():
    for root in (os.environ.get("ROCM_PATH"), os.environ.get("HIP_PATH"), "/opt/rocm"):
        if root and os.path.exists(os.path.join(root, "include", "hip", "hip_runtime_api.h")):
            return os.path.join(root, "include")
    raise AssertionError("hip/hip_runtime_api.h not found (ROCM_PATH, HIP_PATH, /opt/rocm)")


def test_owners_free_everything_once_on_every_way_out(tmp_path):
    exe = str(tmp_path / "scratch_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    "-I" + _hip_include(), "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "host", "scratch_main.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok"), run.stdout + run.stderr
