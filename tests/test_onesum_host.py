"""CPU tier: one column block of phase 2 of the site-fused sweep in its one-sum form (csrc/qk_fused.h: qkf_p2_onesum) --
tests/host_san/onesum_main.cpp, built with -fsanitize=address,undefined and run as a program, restates the block in plain C++ on random
16 x 16 x (4 kmax) complex operands: the ordinary identity (X' += T^T conj(A)) and the switch identity (X'^H = conj(T)^T A, source
operands exchanged) with ONE operand sum per fragment element, the chain of k1 started on zero and the chains of re and im started on
k1; kmax = 1 .. 4, the full and the ragged form, a single tile and a pair; the T-side sets taken from the three real products of phase 1
and from the tile (re, im).  Each against the straightforward complex product to 1e-13 of sum |T| |A|, and the switch result against the
conjugate transpose of the ordinary one.  No GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_onesum_block(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "onesum")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "host_san", "onesum_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(run.stdout, run.stderr[-2000:])
    assert run.returncode == 0 and "FAIL" not in run.stdout, run.stdout + run.stderr[-2000:]
    assert run.stdout.count("ok  ") == 3, run.stdout
    counts = {m.group(1): int(m.group(2)) for m in re.finditer(r"(\w+): (\d+) checked, 0 bad", run.stdout)}
    blocks = 24 * 5 * 3 * 2  # draws x (kmax 1 .. 4 ragged, 4 full) x tiles (a single one, the two of a pair) x derivations of the sets
    assert counts == {"ordinary": blocks * 256, "switch": blocks * 256, "adjoint": blocks * 256}, counts
