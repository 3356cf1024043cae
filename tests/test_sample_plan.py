"""CPU tier: the host-side plan of the measurement shots (csrc/qk_local_plan.h, the SMP_* kinds) under AddressSanitizer and UBSan, by
the stand-alone program tests/host_san/sample_plan_main.cpp -- Philox against its known answers, the shot tiles of a state (every
shot once, ragged tails), the regions of a chain's slot against what the launches index, the task counts, the launch lists of a
chain batch that does not start at chain 0, the same work for any cut into chain batches, the environment pass that keeps the
right environments only and the check of the basis codes, without a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sample_plan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "sample_plan")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "host_san", "sample_plan_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "FAIL" not in run.stdout, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.count("ok  ") == 8, run.stdout
