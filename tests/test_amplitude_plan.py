"""CPU tier: the host-side plan of the amplitude chains (csrc/qk_local_plan.h, the AMP_* kinds) under AddressSanitizer and UBSan, by
the stand-alone program tests/host_san/amplitude_plan_main.cpp -- the string tiles of a state (every string once, ragged tails), the
regions of a chain's slot against what the launches index, the task counts and the launch count, the launch lists of a chain batch
that does not start at chain 0, the same work for any cut into chain batches, the state batch with and without the environment
pass, the check of the outcome bytes and the log likelihood of a mantissa and an exponent, without a GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_amplitude_plan(tmp_path):
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ (what the build itself compiles the planner with) is not on the PATH"
    exe = str(tmp_path / "amplitude_plan")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "host_san", "amplitude_plan_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "FAIL" not in run.stdout, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.count("ok  ") == 7, run.stdout
