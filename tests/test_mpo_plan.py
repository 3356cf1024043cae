"""CPU tier: the plan side of the MPO observables (csrc/qk_local_plan.h: mpo_plan, mpo_task_count, list_mpo_chains, mpo_lists) under
AddressSanitizer and UBSan, by the stand-alone program tests/host_san/mpo_plan_main.cpp -- supports, block lists (order, zero
blocks dropped, a v without a block), slot regions, the task counts of the four launch kinds, and chain cuts that cover every chain
once, without a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mpo_plan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "mpo_plan")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "host_san", "mpo_plan_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "FAIL" not in run.stdout, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.count("ok  ") == 3, run.stdout
