"""GPU tier: the column blocks of phase 2 of the site-fused sweep in their one-sum form (csrc/qk_fused.h: qkf_p2_onesum, qkf_p2_blocks) --
ordinary steps (X' += T^T conj(A)) and switch steps (X'^H = conj(T)^T A) run ONE block body: one operand sum per fragment element, the
chains of re and im started on k1, the fragment registers reloaded late or in a second set (the form is chosen per launch shape).

States: general-gauge twins (tests/helpers.py: scrambled) of random_mps on chains of 16 sites: the bond rows of tests/test_gpu_assoc.py
plus one x row and one y row with bonds of 12, 14, 28, 44, 56 and 80 (column-block counts of 1 .. 6, last groups of 1, 2, 3 and 4
k-steps, a bond of 14 inside one k-step).  Every launch shape (the 12-wave dual kernel, the one-tile kernel with 12 and with 8 waves)
with QK_EDGE=0 (the whole chain) and QK_EDGE=4.  What the blocks meet is ASSERTED from the function the device runs, compiled for the
host (tools/merge_potential.py: onesum_pairs), for the ordinary and for the switch steps separately: 1, 2, an odd number >= 3 and an even
number >= 4 of column blocks (the last block reloading from the next unit; the second half of a ping-pong trip entered first), last
groups of 1, 2, 3 and 4 k-steps, single tiles and pairs of tiles (dual kernel), merged and plain steps, and -- ordinary steps -- a strip
step (96 x 96).

z and |z|^2 of QK_ASSOC=0, 1, 2, 3 against the oracle at 1e-11, against each other at 1e-13, and each against the QK_DETERMINISTIC=1
Gram (ordered kernels, which keep the first 3M form) at 1e-13; launches of 1 pair and of 2 grid + 1 pairs."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-11
SWEEP_EPS = 1e-13
N = 16
SHAPES = {  # shape: (switches, kernel, shape name of tools/merge_potential.py)
    "dual": ({"QK_FUSED_WGS": "1", "QK_FUSED_DUAL": "1"}, "qk_sweep_fused_dual_kernel<12, 8192, 3, {det}>", "12-wave dual (XCAP 8192)"),
    "one-tile": ({"QK_FUSED_WGS": "1", "QK_FUSED_DUAL": "0"}, "qk_sweep_fused_kernel<12, 2, 8192, 3, {det}>", "12-wave one-tile (XCAP 8192)"),
    "two-wg": ({"QK_FUSED_WGS": "2"}, "qk_sweep_fused_kernel<8, 1, 4608, 4, {det}>", "8-wave one-tile (XCAP 4608)"),
}
X_ROWS = [  # true bonds at the cuts 0 .. 16 (a bond is at most twice its neighbours); the first five: tests/test_gpu_assoc.py
    [1, 2, 4, 8, 16, 20, 36, 20, 40, 36, 20, 30, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 16, 32, 64, 96, 96, 64, 36, 20, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 16, 16, 24, 48, 48, 24, 16, 32, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 12, 20, 20, 36, 36, 36, 20, 20, 12, 8, 4, 2, 1],
    [1, 2, 4, 8, 16, 32, 64, 32, 64, 128, 64, 32, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 12, 24, 44, 80, 44, 24, 12, 24, 12, 8, 4, 2, 1],  # 12, 44: last groups of 3 k-steps; 80: five column blocks
]
Y_ROWS = [
    [1, 2, 4, 8, 16, 32, 20, 40, 20, 20, 36, 20, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 16, 32, 48, 96, 96, 48, 32, 20, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 16, 32, 48, 24, 16, 32, 48, 24, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 16, 20, 36, 36, 20, 20, 36, 30, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 16, 28, 56, 80, 40, 20, 40, 28, 14, 8, 4, 2, 1],  # 28: 3 k-steps; 56: 2; 14: the bond ends inside a k-step
]
_cache = {}


def _sets():
    """(xs, ys, z of the oracle [y][x]) -- made once for the module; read-only."""
    import qml_cutensornet_amd as Q
    from helpers import scrambled
    from oracle import c_oracle

    if "sets" not in _cache:
        rng = np.random.default_rng(1020)
        xs = [scrambled(Q.random_mps(N, row, rng), rng) for row in X_ROWS]
        ys = [scrambled(Q.random_mps(N, row, rng), rng) for row in Y_ROWS]
        assert [[int(b) for b in m.bond_dims()] for m in xs] == X_ROWS and [[int(b) for b in m.bond_dims()] for m in ys] == Y_ROWS
        pr = np.array([(i, j) for j in range(len(ys)) for i in range(len(xs))], dtype=np.int32)
        _, z, _ = c_oracle.gram_pairs([m.tensors for m in xs], [m.tensors for m in ys], pr, 8)
        z = z.reshape(len(ys), len(xs))
        z.setflags(write=False)
        _cache["sets"] = (xs, ys, z)
    return _cache["sets"]


def _potential():
    if "tool" not in _cache:
        spec = importlib.util.spec_from_file_location("merge_potential", os.path.join(ROOT, "tools", "merge_potential.py"))
        _cache["tool"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_cache["tool"])
    return _cache["tool"]


def _env(monkeypatch, shape, edge, assoc, det=False):
    for k in ("QK_FUSED_WGS", "QK_FUSED_DUAL", "QK_MERGE", "QK_ASSOC", "QK_SWITCH_PRICE", "QK_FUSED_SPLIT", "QK_PLAN_ORIENT", "QK_GANG"):
        monkeypatch.delenv(k, raising=False)
    for k, v in SHAPES[shape][0].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("QK_FUSED", "2")
    monkeypatch.setenv("QK_PLAN_NO_MIXED", "1")
    monkeypatch.setenv("QK_EDGE", edge)
    monkeypatch.setenv("QK_DETERMINISTIC", "1" if det else "0")
    if assoc is not None:
        monkeypatch.setenv("QK_ASSOC", assoc)
    return SHAPES[shape][1].format(det="true" if det else "false")


def _sweep(monkeypatch, shape, edge, assoc, xs, ys, det=False):
    """(z [y][x], values [y][x], pairs, edge_k, stats) of the rectangular Gram of xs and ys."""
    from qml_cutensornet_amd import engine

    kernel = _env(monkeypatch, shape, edge, assoc, det)
    with engine.context(0) as ctx, ctx.upload(xs) as dx, ctx.upload(ys) as dy:
        plan = engine.Plan(dx.dims, dy.dims, orient=False)
        vals, zz = ctx.gram_values_host(dx, dy, plan, want_z=True)
        st = ctx.stats()
        assert st["kernel_name"] == kernel, st["kernel_name"]
        pairs, ek = plan.pairs(), plan.edge_sites
        plan.close()
    z, v = np.full((len(ys), len(xs)), np.nan + 0j), np.full((len(ys), len(xs)), np.nan)
    z[pairs[:, 1], pairs[:, 0]], v[pairs[:, 1], pairs[:, 0]] = zz, vals
    return z, v, pairs, ek, st


def _visited(tool, shape, pairs, ek):
    """the cases (names of tool.ONESUM_CASES) the ordinary and the switch steps of the four modes meet, from the host function"""
    xd, yd = np.array(X_ROWS, dtype=np.int32), np.array(Y_ROWS, dtype=np.int32)
    seen = [0, 0]
    for a in (0, 1, 2, 3):
        cases, _ = tool.onesum_pairs(xd, yd, pairs, ek, SHAPES[shape][2], a)
        for kind in range(2):
            seen[kind] |= int(np.bitwise_or.reduce(cases[:, kind]))
    return [{name for name, bit in tool.ONESUM_CASES.items() if s & bit} for s in seen]


def _wanted(shape):
    """(of the ordinary steps, of the switch steps): every case, but pairs of tiles exist in the dual kernel only and a switch step is LDS-resident"""
    every = {"nn_1", "nn_2", "nn_odd", "nn_even", "kmax_1", "kmax_2", "kmax_3", "kmax_4", "single_tile", "plain_step", "merged_step"} | ({"tile_pair"} if shape == "dual" else set())
    return every | {"strip_step"}, every


def test_rows_visit_every_case_on_the_host():
    """No GPU needed for this part, but it belongs to the rows: the cases are visited whatever edge_k the plan picks (0 and 4 are what the tests set)."""
    tool = _potential()
    pairs = np.array([(i, j) for j in range(len(Y_ROWS)) for i in range(len(X_ROWS))], dtype=np.int32)
    for shape in SHAPES:
        for ek in (0, 4):
            got, want = _visited(tool, shape, pairs, ek), _wanted(shape)
            assert want[0] <= got[0] and want[1] <= got[1], (shape, ek, want[0] - got[0], want[1] - got[1])


@pytest.mark.parametrize("edge", ["0", "4"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_one_sum_blocks_agree_with_the_oracle_the_modes_and_the_ordered_kernels(built, monkeypatch, shape, edge):
    xs, ys, z_ref = _sets()
    tool = _potential()
    out = {a: _sweep(monkeypatch, shape, edge, a, xs, ys) for a in ("0", "1", "2", "3")}
    zd, vd, _, _, _ = _sweep(monkeypatch, shape, edge, "0", xs, ys, det=True)  # the ordered kernels: this form is not in them
    pairs, ek = out["1"][2], out["1"][3]
    assert ek == int(edge) and len(pairs) == len(xs) * len(ys)
    assert np.abs(zd - z_ref).max() < TOL
    for a, (z, v, _, _, _) in out.items():
        print(f"{shape} QK_EDGE={edge} QK_ASSOC={a}: max |z - oracle| {np.abs(z - z_ref).max():.2e}, |values - oracle| {np.abs(v - np.abs(z_ref) ** 2).max():.2e}, "
              f"|z - QK_ASSOC=0| {np.abs(z - out['0'][0]).max():.2e}, |z - ordered| {np.abs(z - zd).max():.2e}")
        assert np.abs(z - z_ref).max() < TOL and np.abs(v - np.abs(z_ref) ** 2).max() < TOL
        assert np.abs(z - out["0"][0]).max() < SWEEP_EPS and np.abs(v - out["0"][1]).max() < SWEEP_EPS
        assert np.abs(z - zd).max() < SWEEP_EPS and np.abs(v - vd).max() < SWEEP_EPS
    got, want = _visited(tool, shape, pairs, ek), _wanted(shape)
    print(f"{shape} QK_EDGE={edge}: ordinary steps meet {sorted(got[0])}, switch steps {sorted(got[1])}")
    assert want[0] <= got[0], want[0] - got[0]
    assert want[1] <= got[1], want[1] - got[1]


def _factors(m):
    nx = int(m ** 0.5)
    while m % nx:
        nx -= 1
    return m // nx, nx


@pytest.mark.parametrize("wgs", [1, 2])
def test_launches_of_one_pair_and_of_two_grids_plus_one(built, monkeypatch, wgs):
    """1 pair (most workgroups get none) and 2 grid + 1 pairs (a workgroup takes several pairs, one of them a third: the fragment registers
    are handed from the last block of a pair's last unit to nothing, and the next pair starts unprimed)."""
    import torch

    shape = "dual" if wgs == 1 else "two-wg"
    grid = wgs * torch.cuda.get_device_properties(0).multi_processor_count
    nx, ny = _factors(2 * grid + 1)
    xs6, ys5, z65 = _sets()
    ix, iy = [(5 * i) % len(xs6) for i in range(nx)], [(i + i // len(ys5)) % len(ys5) for i in range(ny)]
    for cx, cy in ((1, 1), (nx, ny)):
        xs, ys = [xs6[i] for i in ix[:cx]], [ys5[j] for j in iy[:cy]]
        z_ref = z65[np.ix_(iy[:cy], ix[:cx])]
        zd, vd, _, _, _ = _sweep(monkeypatch, shape, "0", "0", xs, ys, det=True)
        z0, v0, _, _, st = _sweep(monkeypatch, shape, "0", "0", xs, ys)
        assert st["pairs"] == cx * cy and (cx * cy == 1 or st["pairs"] == 2 * st["grid"] + 1), st
        for a in ("0", "1", "2"):
            z, v, _, _, _ = _sweep(monkeypatch, shape, "0", a, xs, ys)
            assert np.abs(z - z_ref).max() < TOL and np.abs(v - np.abs(z_ref) ** 2).max() < TOL, (cx, cy, a)
            assert np.abs(z - z0).max() < SWEEP_EPS and np.abs(v - v0).max() < SWEEP_EPS, (cx, cy, a)
            assert np.abs(z - zd).max() < SWEEP_EPS and np.abs(v - vd).max() < SWEEP_EPS, (cx, cy, a)
