"""CPU tier: the segmentation of a pair's chain into plain and merged steps (qk_segment_chain, csrc/qk_plan.h) --
tests/host_san/segment_main.cpp, built with -fsanitize=address,undefined, checks that the dynamic programme reaches the brute-force
minimum of the objective over all admissible segmentations with a well-formed mask (chains of 1 .. 12 middle sites, n - 2 k odd and
even, k = 0 and 4, a chain of 2 middle sites, all three launch shapes, every mask of allowed parities), that with odd starts
disallowed and every admissible merge taken the mask is the rule the step table applied before (the anchor of QK_MERGE=1, every pair
of 40 random states), and that the programme is never worse than that rule under the objective.  No GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segment_chain(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "segment")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "host_san", "segment_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(run.stdout, run.stderr[-2000:])
    assert run.returncode == 0 and "FAIL" not in run.stdout, run.stdout + run.stderr[-2000:]
    assert run.stdout.count("ok  ") == 3, run.stdout
    counts = {m.group(1): int(m.group(2)) for m in re.finditer(r"(\w+): (\d+) checked, 0 bad", run.stdout)}
    # 3 shapes x 4 parity masks x (7^2 + 7^3 + 7^4 + 7^5 exhaustive + 12 lengths x 2 k x 1500 drawn); one comparison per shape and chain; 40 x 40 pairs x 3 shapes x 7 (n, k)
    assert counts == {"dp": 12 * (19600 + 36000), "never_worse": 3 * (19600 + 36000), "anchor": 1600 * 3 * 7}, counts
