"""CPU tier: the integer side of the shot-based block overlaps (csrc/qk_local_plan.h, sbk_*) under AddressSanitizer and UBSan, by the
stand-alone program tests/host_san/shot_block_main.cpp -- the mask and the term at w = 1, 31 and 32 (the shift at 32 is what UBSan is
there for) and the double the kernel adds, the packed word at n = 1, 32 and 33 on both sides, the task cut that covers every (pair,
setting) once for several chunk sizes, the chunk against what a workgroup stages, the pieces of a staged row, the groups of widths and
the overflow rule at its boundary, without a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shot_block_plan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "shot_block")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "host_san", "shot_block_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "FAIL" not in run.stdout, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.count("ok  ") == 7, run.stdout
