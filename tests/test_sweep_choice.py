"""CPU tier: the sweep's choice of launches (qk_choose_sweep, csrc/qk_plan.h) against the table of tests/host_san/choice_main.cpp --
kernel, grid, dynamic LDS, pairs of each launch and scratch bytes for the product build's switches, without a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweep_choice_table(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "choice")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "host_san", "choice_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "FAIL" not in run.stdout, run.stdout
    assert run.stdout.count("ok  ") == 24, run.stdout
