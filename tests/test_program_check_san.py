"""CPU tier: the one validation of a gate program (csrc/qk_program.h), shared by the device and the host builder, built with
AddressSanitizer + UndefinedBehaviorSanitizer and driven by tests/host_san/program_check_main.cpp, a stand-alone program -- the recipe
of tests/test_conditions_san.py.  The driver runs no builder and needs no LAPACK."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_program_check_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "program_check_san")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
           os.path.join(ROOT, "tests", "host_san", "program_check_main.cpp")]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and ("cannot find" in build.stderr or "unrecognized" in build.stderr):
        pytest.skip("this toolchain has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    # 8 matrix-gate, 12 channel, 12 two-qubit-channel and 8 condition rejections, 4 with the fault in state 1 of two
    assert "accepted: exact tables, 1 and 2 states" in run.stdout and "44 rejections ok, 0 missed" in run.stdout, run.stdout
