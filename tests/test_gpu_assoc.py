"""GPU tier: the association of the steps of the site-fused sweep (QK_ASSOC; csrc/qk_plan.h: qk_segment_chain, csrc/qk_fused.h:
qkf_p2_switch) -- a step may leave X'^H and hand the chain to the other orientation ("A first": the two states exchanged, W = X^H).
The complex overlaps z AND the values |z|^2 of QK_ASSOC=0 (orientation 0 throughout), 1 (the dynamic programme, the default), 2 and 3
(test patterns: a switch behind every step that may switch, starting in orientation 0 / 1) against the oracle at 1e-11 and against
each other at 1e-13.

States: general-gauge twins (tests/helpers.py: scrambled) of random_mps on chains of 16 sites with the crafted bond rows X_ROWS and
Y_ROWS below (a rectangular Gram: x set != y set): zigzags in opposite phase, so that the cheaper association changes along the chain
and the programme really switches; bonds 20, 30 and 36 (no multiples of 16: k-tails of 1 .. 3 k-steps, odd tile counts, single tiles
beside pairs); one pair of rows with 96 x 96 in the middle, above the 8192-element buffer (strip steps between two switches); an x
row with a dip that forbids the merges around a step whose X and X' do not fit side by side (a switch on a one-round step).  With
QK_EDGE=0 the whole chain is walked, with QK_EDGE=4 the sites 4 .. 11 between the edge blocks (which are then taken with the states
exchanged where the chain starts or ends in orientation 1).  What the cases cover is ASSERTED from the function the device runs,
compiled for the host (tools/merge_potential.py: assoc_pairs): the programme switches, chains start and end in orientation 1, and the
patterns put a switch on the first and on the last step, on a merged step, on a one-round step, on a ping-pong step and around strip
steps.  All three launch shapes (the 12-wave dual kernel, the one-tile kernel with 12 and with 8 waves).  Further: a symmetric Gram, launches
of 1 pair and of 2 grid + 1 pairs, and QK_DETERMINISTIC=1, which ignores QK_ASSOC and keeps its bits."""
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
X_ROWS = [  # true bonds at the cuts 0 .. 16 (a bond is at most twice its neighbours)
    [1, 2, 4, 8, 16, 20, 36, 20, 40, 36, 20, 30, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 16, 32, 64, 96, 96, 64, 36, 20, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 16, 16, 24, 48, 48, 24, 16, 32, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 12, 20, 20, 36, 36, 36, 20, 20, 12, 8, 4, 2, 1],
    [1, 2, 4, 8, 16, 32, 64, 32, 64, 128, 64, 32, 16, 8, 4, 2, 1],  # the dip at cut 7 forbids the merges around site 7: against Y_ROWS[1] a one-round step
]
Y_ROWS = [
    [1, 2, 4, 8, 16, 32, 20, 40, 20, 20, 36, 20, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 16, 32, 48, 96, 96, 48, 32, 20, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 16, 32, 48, 24, 16, 32, 48, 24, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 16, 20, 36, 36, 20, 20, 36, 30, 16, 8, 4, 2, 1],
]
_cache = {}


def _sets():
    """(xs, ys, z of the oracle [y][x]) -- made once for the module; read-only."""
    import qml_cutensornet_amd as Q
    from helpers import scrambled
    from oracle import c_oracle

    if "sets" not in _cache:
        rng = np.random.default_rng(916)
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
    """(z [y][x], values [y][x], pairs, edge_k, stats) of the rectangular Gram of xs and ys (ys None: the symmetric one of xs)."""
    from qml_cutensornet_amd import engine

    kernel = _env(monkeypatch, shape, edge, assoc, det)
    with engine.context(0) as ctx, ctx.upload(xs) as dx:
        dy = ctx.upload(ys) if ys is not None else None
        plan = engine.Plan(dx.dims, None if dy is None else dy.dims, orient=False)
        vals, zz = ctx.gram_values_host(dx, dy, plan, want_z=True)
        st = ctx.stats()
        assert st["kernel_name"] == kernel, st["kernel_name"]
        pairs, ek = plan.pairs(), plan.edge_sites
        plan.close()
        if dy is not None:
            dy.close()
    ny = len(xs) if ys is None else len(ys)
    z, v = np.full((ny, len(xs)), np.nan + 0j), np.full((ny, len(xs)), np.nan)
    z[pairs[:, 1], pairs[:, 0]], v[pairs[:, 1], pairs[:, 0]] = zz, vals
    return z, v, pairs, ek, st


def _flags(tool, fl):
    every = 0
    for f in fl:
        every |= int(f)
    return {name for name, bit in tool.ASSOC_FLAGS.items() if every & bit}


@pytest.mark.parametrize("edge", ["0", "4"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_switch_steps_agree_with_the_oracle_and_with_orientation_0(built, monkeypatch, shape, edge):
    xs, ys, z_ref = _sets()
    tool = _potential()
    out = {a: _sweep(monkeypatch, shape, edge, a, xs, ys) for a in ("0", "1", "2", "3")}
    z_def = _sweep(monkeypatch, shape, edge, None, xs, ys)[0]
    pairs, ek = out["1"][2], out["1"][3]
    assert ek == int(edge) and len(pairs) == len(xs) * len(ys)
    xd, yd = np.array(X_ROWS, dtype=np.int32), np.array(Y_ROWS, dtype=np.int32)
    host = {a: tool.assoc_pairs(xd, yd, pairs, ek, SHAPES[shape][2], int(a)) for a in out}
    for a, (z, v, _, _, _) in out.items():
        print(f"{shape} QK_EDGE={edge} QK_ASSOC={a}: max |z - oracle| {np.abs(z - z_ref).max():.2e}, |values - oracle| {np.abs(v - np.abs(z_ref) ** 2).max():.2e}, "
              f"|z - QK_ASSOC=0| {np.abs(z - out['0'][0]).max():.2e}; switches per pair {host[a][3].tolist()}, {sorted(_flags(tool, host[a][4]))}")
        assert np.abs(z - z_ref).max() < TOL and np.abs(v - np.abs(z_ref) ** 2).max() < TOL
        assert np.abs(z - out["0"][0]).max() < SWEEP_EPS and np.abs(v - out["0"][1]).max() < SWEEP_EPS
    assert np.abs(z_def - out["1"][0]).max() < SWEEP_EPS  # the default is the programme
    # what the cases cover, from the host function: orientation 0 never switches; the programme really switches and chains start and
    # end in orientation 1; the patterns switch on the first and on the last step, on a merged step, on a one-round and on a ping-pong step
    assert host["0"][3].sum() == 0 and not host["0"][0][:, 2:].any()
    assert host["1"][3].sum() > 0 and {"starts_o1", "ends_o1"} <= _flags(tool, host["1"][4])
    pattern = _flags(tool, host["2"][4]) | _flags(tool, host["3"][4])
    assert {"starts_o1", "ends_o1", "first_step", "last_step", "merged_step", "pingpong_step"} <= pattern, pattern
    assert host["2"][3].sum() > host["1"][3].sum() and not (host["2"][4] & 1).any() and (host["3"][4] & 1).all()
    if shape != "two-wg":  # (bonds up to 48 next to each other: in place in the 8192-element buffer; strips only for the pair of 96 x 96)
        assert {"one_round_step", "strip_between"} <= pattern, pattern


@pytest.mark.parametrize("shape", list(SHAPES))
def test_symmetric_gram_with_switch_steps(built, monkeypatch, shape):
    """x set = y set (the four x states and two y states in one set): every pair (i, j), i <= j, in the order the plan lists it."""
    from oracle import c_oracle

    xs, ys, _ = _sets()
    states = xs + ys[2:]
    if "sym" not in _cache:
        pr = np.array([(i, j) for j in range(len(states)) for i in range(len(states))], dtype=np.int32)
        _, z, _ = c_oracle.gram_pairs([m.tensors for m in states], None, pr, 8)
        _cache["sym"] = z.reshape(len(states), len(states))
    z_ref = _cache["sym"]
    z0, v0, pairs, _, _ = _sweep(monkeypatch, shape, "4", "0", states, None)
    got = ~np.isnan(v0)
    assert got.sum() == len(states) * (len(states) + 1) // 2
    for a in ("1", "2"):
        z, v, _, _, _ = _sweep(monkeypatch, shape, "4", a, states, None)
        assert np.array_equal(~np.isnan(v), got)
        print(f"{shape} symmetric QK_ASSOC={a}: max |z - oracle| {np.abs(z - z_ref)[got].max():.2e}, |z - QK_ASSOC=0| {np.abs(z - z0)[got].max():.2e}")
        assert np.abs(z - z_ref)[got].max() < TOL and np.abs(v - np.abs(z_ref) ** 2)[got].max() < TOL
        assert np.abs(z - z0)[got].max() < SWEEP_EPS and np.abs(v - v0)[got].max() < SWEEP_EPS


@pytest.mark.parametrize("edge", ["0", "4"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_deterministic_mode_ignores_the_association(built, monkeypatch, shape, edge):
    """QK_DETERMINISTIC=1 runs the ordered kernels, which have no switch step: QK_ASSOC is ignored and the bits are those of QK_ASSOC=0."""
    xs, ys, z_ref = _sets()
    z0, v0, _, _, _ = _sweep(monkeypatch, shape, edge, "0", xs, ys, det=True)
    for a in ("2", None):
        z, v, _, _, _ = _sweep(monkeypatch, shape, edge, a, xs, ys, det=True)
        assert np.array_equal(z, z0) and np.array_equal(v, v0)
    assert np.abs(z0 - z_ref).max() < TOL


def _factors(m):
    nx = int(m ** 0.5)
    while m % nx:
        nx -= 1
    return m // nx, nx


@pytest.mark.parametrize("wgs", [1, 2])
def test_launches_of_one_pair_and_of_two_grids_plus_one(built, monkeypatch, wgs):
    """1 pair (most workgroups get none) and 2 grid + 1 pairs (every workgroup reads the four mask words of several pairs, one of them a
    third): the masks of a pair are found at the pair's index in the launch's list.  The rows alternate, so neighbouring pairs differ in
    their orientations."""
    import torch

    shape = "dual" if wgs == 1 else "two-wg"
    grid = wgs * torch.cuda.get_device_properties(0).multi_processor_count
    nx, ny = _factors(2 * grid + 1)
    xs4, ys4, z4 = _sets()
    ix, iy = [(3 * i) % 4 for i in range(nx)], [(i + i // 4) % 4 for i in range(ny)]
    for cx, cy in ((1, 1), (nx, ny)):
        xs, ys = [xs4[i] for i in ix[:cx]], [ys4[j] for j in iy[:cy]]
        z_ref = z4[np.ix_(iy[:cy], ix[:cx])]
        z0, v0, _, _, st = _sweep(monkeypatch, shape, "0", "0", xs, ys)
        assert st["pairs"] == cx * cy and (cx * cy == 1 or st["pairs"] == 2 * st["grid"] + 1), st
        for a in ("1", "2"):
            z, v, _, _, _ = _sweep(monkeypatch, shape, "0", a, xs, ys)
            assert np.abs(z - z_ref).max() < TOL and np.abs(v - np.abs(z_ref) ** 2).max() < TOL, (cx, cy, a)
            assert np.abs(z - z0).max() < SWEEP_EPS and np.abs(v - v0).max() < SWEEP_EPS, (cx, cy, a)
