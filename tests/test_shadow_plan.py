"""CPU tier: the integer side of the shadow kernel's shot-pair histograms (csrc/qk_local_plan.h, shk_*) under AddressSanitizer and
UBSan, by the stand-alone program tests/host_san/shadow_main.cpp -- the record packer and d at n = 1, 32, 33, 64, 65 and 128, the task
cut that covers every (pair, x block) once, the counter bound at its boundary, the LDS layout for every n up to 128 against the 160 KiB
of a CU, the pieces of a staged pass and the pairs of a batch, without a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shadow_plan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "shadow")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "host_san", "shadow_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "FAIL" not in run.stdout, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.count("ok  ") == 6, run.stdout
