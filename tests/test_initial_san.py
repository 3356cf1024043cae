"""CPU tier: building from a given state in the native host MPS builder (csrc/qk_builder.cpp: qkb_simulate_program, spelt qkb_simulate_initial in tests/host_san/qkb_calls.h) built with
AddressSanitizer + UndefinedBehaviorSanitizer and driven by tests/host_san/initial_main.cpp, a stand-alone program -- the recipe
of tests/test_conditions_san.py."""
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qml-cutensornet_amd", "csrc")


def test_initial_states_of_the_host_builder_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "initial_san")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
           "-o", exe, os.path.join(ROOT, "tests", "host_san", "initial_main.cpp"), os.path.join(CSRC, "qk_builder.cpp"), "-ldl"]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and ("cannot find" in build.stderr or "unrecognized" in build.stderr):
        pytest.skip("this toolchain has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    import scipy

    blas = sorted(glob.glob(os.path.join(os.path.dirname(scipy.__file__), "..", "scipy.libs", "libscipy_openblas*.so*")))
    assert blas, "the OpenBLAS that scipy ships was not found"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe, os.path.realpath(blas[0])], capture_output=True, text=True, env=env, timeout=600)
    assert run.returncode == 0, (run.returncode, run.stdout[-1000:], run.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    assert "product state: max deviation" in run.stdout and "split run: max deviation" in run.stdout and "8 rejections ok" in run.stdout, run.stdout
