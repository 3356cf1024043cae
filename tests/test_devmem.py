"""CPU tier: the owners of device memory (QkDevBuf / QkGrowBuf, csrc/qk_devmem.h) over a counting malloc-backed allocator, built with
AddressSanitizer + UndefinedBehaviorSanitizer and run with leak detection (tests/host_san/devmem_main.cpp): moves, release(), ensure()
and what is left alive when the n-th allocation of a call fails."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_device_memory_owners_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "devmem")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-o", exe, os.path.join(ROOT, "tests", "host_san", "devmem_main.cpp")]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and ("cannot find" in build.stderr or "unrecognized" in build.stderr):
        pytest.skip("this toolchain has no sanitizer runtime")
    assert build.returncode == 0 and "warning" not in build.stderr, build.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert run.returncode == 0 and "FAIL" not in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-3000:])
    assert "devmem: all cases passed" in run.stdout and run.stdout.count("ok   fail allocation") == 8, run.stdout
    assert "ERROR: AddressSanitizer" not in run.stderr and "LeakSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
