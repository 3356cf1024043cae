"""CPU tier: the plan side of the strings of single-site operators (csrc/qk_local_plan.h: operator_supports) under AddressSanitizer
and UBSan, by the stand-alone program tests/host_san/op_strings_main.cpp -- supports with codes up to 255, the index of the first
code above n_ops, string_supports as the n_ops = 3 case, and chains, weights, cuts and task lists equal to those of the Pauli
strings with the same zeros, without a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_op_strings_plan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "op_strings_plan")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "host_san", "op_strings_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "FAIL" not in run.stdout, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.count("ok  ") == 2, run.stdout
