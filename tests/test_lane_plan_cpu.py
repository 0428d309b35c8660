"""The host half of a multi-lane learn (csrc/lane_plan.hpp) on the CPU.

The plan is plain integer and scalar functions shared by engine::learn_held and tests/lane_plan_check.cpp; this test
builds that program with the host compiler and runs it: the argument checks with their codes and texts, pivots, pivot
groups in both lane orders, masks, right-hand sides, QA in its three weight cases and the end of learn() with the pivot
as a parameter, each in float and double with ==. A second build runs under the address and undefined-behaviour
sanitizers, as a plain executable.
"""
import os
import subprocess

import pytest

from test_kp_record_cpu import SANITIZE, _cxx, _has_sanitizer_runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "lane_plan_check.cpp")
INC = os.path.join(ROOT, "plssvm_sparse_fp22_amd", "csrc")


def _build_and_run(exe, flags):
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", INC, SRC, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok"), run.stdout


def test_lane_plan(tmp_path):
    _build_and_run(tmp_path / "lane_plan_check", [])


def test_lane_plan_under_sanitizers(tmp_path):
    if not _has_sanitizer_runtime(tmp_path):
        pytest.skip("the host compiler has no address / undefined-behaviour sanitizer runtime")
    _build_and_run(tmp_path / "lane_plan_check_san", SANITIZE)
