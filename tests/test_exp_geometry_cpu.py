"""The host decisions of the kernel expansion's setup (csrc/exp_geometry.hpp) on the CPU.

The remainder stream's geometry (accumulator class, rows per block, window groups, window), the slot cap of the one-pass
joins and the two layout rules are plain integer functions shared by csrc/expand_setup.hip and
tests/exp_geometry_check.cpp; this test builds that program with the host compiler and runs it: the two timed
geometries, every accumulator class boundary for fp32 and fp64, R = 0 and 1, the forcing knobs and the rules at equality
and to either side, all as literals. A second build runs under the address and undefined-behaviour sanitizers, as a
plain executable.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "exp_geometry_check.cpp")
INC = os.path.join(ROOT, "plssvm_sparse_fp22_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _cxx():
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    return cxx


def _build_and_run(exe, flags):
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", INC, SRC, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok"), run.stdout


def test_exp_geometry_decisions(tmp_path):
    _build_and_run(tmp_path / "exp_geometry_check", [])


def _has_sanitizer_runtime(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([_cxx(), *SANITIZE, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    return r.returncode == 0 and subprocess.run([str(tmp_path / "probe")]).returncode == 0


def test_exp_geometry_decisions_under_sanitizers(tmp_path):
    if not _has_sanitizer_runtime(tmp_path):
        pytest.skip("the host compiler has no address / undefined-behaviour sanitizer runtime")
    _build_and_run(tmp_path / "exp_geometry_check_san", SANITIZE)
