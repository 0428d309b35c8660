"""The 7-byte record format of stored fp64 tiles (csrc/kp_pack.hpp) on the CPU.

The format is plain integer functions shared by the store kernel, the load kernel and tests/kp_pack_check.cpp; this
test builds that program with the host compiler and runs it: classification of tiles (raw / packed), bit-exact round
trips, and the kernels' 4-values-into-7-dwords grouping.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kp_pack_format(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    exe = tmp_path / "kp_pack_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "plssvm_sparse_fp22_amd", "csrc"),
                    os.path.join(ROOT, "tests", "kp_pack_check.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok"), run.stdout
