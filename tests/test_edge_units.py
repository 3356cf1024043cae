"""CPU tier: the units of an edge product in the site-fused sweep (qk_edge_units / qk_edge_unit, csrc/qk_plan.h) --
tests/host_san/edge_units_main.cpp checks, for every mt, nt in 1..16 and NW in {8, 12}, that the decode covers every tile exactly once,
pairs only tiles of one row block and neighbouring column blocks, and deals the last round as single tiles exactly when its pairs fill
at most half of the waves.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_edge_units():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "edge_units")
        build = subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "host_san", "edge_units_main.cpp")], capture_output=True, text=True)
        assert build.returncode == 0, build.stderr[-2000:]
        run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0 and "FAIL" not in run.stdout, run.stdout
    assert run.stdout.count("ok  ") == 4, run.stdout
    assert run.stdout.count("512 checked, 0 bad") == 4, run.stdout  # 2 NW x 16 x 16 shapes
