"""CPU tier: the host-side plan of the k-qubit windows (csrc/qk_local_plan.h: the WIN_* kinds) under AddressSanitizer and UBSan,
by the stand-alone program tests/host_san/window_plan_main.cpp -- the slot layout, the pair index of the closing sums, the task
counts, every output block of every launch listed exactly once for ragged bonds and several cuts into chain batches, the tables
of a batch other than the first, and the checks of width and starts, without a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_plan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "window_plan")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "host_san", "window_plan_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "FAIL" not in run.stdout, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.count("ok  ") == 5, run.stdout
