"""CPU tier: the association of the steps of a pair's chain (qk_segment_chain with assoc, qk_step_record; csrc/qk_plan.h) --
tests/host_san/assoc_main.cpp, built with -fsanitize=address,undefined and run as a program, checks that the dynamic programme over
(site, orientation) reaches the brute-force lexicographic minimum of (objective, switches, steps in orientation 1, steps) over all
segmentations with orientations (chains of 1 .. 10 middle sites, k = 0 and 3, all three launch shapes, switch prices 0, 40 and 150)
with well-formed masks and no switch behind a step that is not LDS-resident, that assoc = 0 gives the masks of the segmentation as it
was before, bit for bit, that x = y never switches, that the test patterns switch wherever a switch is allowed, that a chain without
room for the end bit keeps orientation 0, that the step-table record of an orientation-1 step is the orientation-0 record of the
exchanged pair, and the two 3M forms of phase 2 on random complex numbers.  No GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_assoc_chain(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "assoc")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "host_san", "assoc_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(run.stdout, run.stderr[-2000:])
    assert run.returncode == 0 and "FAIL" not in run.stdout, run.stdout + run.stderr[-2000:]
    assert run.stdout.count("ok  ") == 7, run.stdout
    counts = {m.group(1): int(m.group(2)) for m in re.finditer(r"(\w+): (\d+) checked, 0 bad", run.stdout)}
    chains = 2 * 10 * 60 * 3  # k x lengths x draws x shapes
    assert counts == {"dp": chains * 3, "pattern": chains * 2, "assoc0": chains * 8, "symmetric": 10 * 40 * 3 * 2, "long": 9, "record": 400 * 3 * 8, "3m": 20000}, counts
