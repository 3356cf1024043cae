"""CPU tier: the plan side of applying an MPO to a set (csrc/qk_local_plan.h: apply_plan) under AddressSanitizer and UBSan, by the
stand-alone program tests/host_san/apply_plan_main.cpp -- new bonds, pads and 64-bit offsets of ragged sets, the row lists of the
blocks (zero blocks absent, identity sites marked as copies), tasks that cover every (state, site, u, chunk) and every double of the
image exactly once, the 512 limit and offsets beyond 2^31 doubles, without a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_apply_plan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "apply_plan")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "host_san", "apply_plan_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "FAIL" not in run.stdout, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.count("ok  ") == 3, run.stdout
