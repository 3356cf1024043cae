"""CPU tier: the host-side plan of the block kernels (csrc/qk_local_plan.h, the BLK_* kinds) under AddressSanitizer and UBSan, by the
stand-alone program tests/host_san/block_plan_main.cpp -- the geometry of a step for both sides, the pair-chain task counts over
rectangular bonds, the slot regions (V and W inside T), the launches of a width list that skips cuts, the offsets of the kept-cut
buffer, the cut into several pair batches and the task lists of a batch that does not start at pair 0, without a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_block_plan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "block_plan")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "host_san", "block_plan_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "FAIL" not in run.stdout, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.count("ok  ") == 6, run.stdout
