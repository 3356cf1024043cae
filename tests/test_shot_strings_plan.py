"""CPU tier: the integer side of the Pauli-string estimator (csrc/qk_local_plan.h, sst_*) under AddressSanitizer and UBSan, by the
stand-alone program tests/host_san/shot_strings_main.cpp -- the string packer at n = 1, 31, 32, 33, 64, 65 and 128, match and sign of
a (shot record, string record) against a loop over the qubits, the task cut that covers every (state, string block, shot) once, the
int32 overflow bound at its boundary and the strings of a batch, without a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shot_strings_plan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "shot_strings")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "host_san", "shot_strings_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "FAIL" not in run.stdout, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.count("ok  ") == 5, run.stdout
