"""CPU tier: the residency of X in a step of the site-fused sweep (qk_resident, qk_rec_resident, qk_res_global_mask; csrc/qk_plan.h) --
tests/host_san/resident_main.cpp, built with -fsanitize=address,undefined and run as a program, checks exhaustively over the padded bonds
16 .. 256 in steps of 16, pd 2 and 4, X at either end of the buffer and the launch shapes (the 12-wave shapes with the large buffer and with
the segmentation's, the 8-wave shape) that X' and the panels of X that stay never overlap and lie inside the buffer, that as many panels stay
as fit, that side-by-side steps keep every panel, that a step which does not fit keeps nothing, that the rule with the segmentation's
buffer and without partial residency is the classification the kernels had before it, that the step table's word decodes to the rule, and
that qk_choose_sweep gives the large buffer to the 12-wave launches whose tables fit behind it and to no other.
The rows of tests/test_gpu_resident.py are checked here as well: they meet every case that test names, whatever the GPU does.  No GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_residency_rule(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "resident")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "host_san", "resident_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(run.stdout, run.stderr[-2000:])
    assert run.returncode == 0 and "FAIL" not in run.stdout, run.stdout + run.stderr[-2000:]
    assert run.stdout.count("ok  ") == 7 and "choice: the large buffer where the tables fit behind it: 9 checked, 0 bad" in run.stdout, run.stdout
    counts = {m.group(1): int(m.group(2)) for m in re.finditer(r"ok    (\w+): .*: (\d+) checked, 0 bad", run.stdout)}
    assert counts.pop("choice") == 9
    # 5 shapes x 2 pd x 16^4 steps x the ends (the top end only for an X that fits the segmentation's buffer: 861184 - 655360 of them)
    assert set(counts) == {"inside", "apart", "side", "parent", "strips", "record"} and set(counts.values()) == {861184}, counts


def test_rows_of_the_gpu_test_meet_every_case():
    import test_gpu_resident as T

    for case in T.CASES:
        got = T.visited(case)
        assert T.wanted(case) <= got and not (T.never(case) & got), (case, T.wanted(case) - got, T.never(case) & got)
