"""CPU tier: the order of a step's units in the site-fused sweep (qk_unit_decode, csrc/qk_plan.h) -- tests/host_san/units_main.cpp checks,
for pd in {2, 4}, mt and w in 1..32, NW in {8, 12}, dual and one-tile form, that the decode hits every unit exactly once, that the record's
reciprocals equal the divisions, and that the new order never asks for more operand blocks per round than the present one (strictly fewer
with more than one round); then six named steps against their table.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_unit_order():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "units")
        build = subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "host_san", "units_main.cpp")], capture_output=True, text=True)
        assert build.returncode == 0, build.stderr[-2000:]
        run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0 and "FAIL" not in run.stdout, run.stdout
    assert run.stdout.count("ok  ") == 4 + 6, run.stdout
    assert "8192 checked, 0 bad" in run.stdout, run.stdout  # 2 forms x 2 NW x 2 pd x 32 x 32 shapes
