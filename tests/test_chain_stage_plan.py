"""CPU tier: the device buffer of a chain batch (csrc/qk_local_plan.h: chain_stage, chain_stage_max) for the five chain families and
the batch cap of the environment (batch_cap) under AddressSanitizer and UBSan, by the stand-alone program
tests/host_san/chain_stage_main.cpp -- offsets against the restated layout, the image against its sources, zero padding, slot
bases, disjoint regions, the maximum over a cut and the budget bound, without a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_stage_plan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "chain_stage")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "host_san", "chain_stage_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "FAIL" not in run.stdout, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.count("ok  ") == 7, run.stdout
