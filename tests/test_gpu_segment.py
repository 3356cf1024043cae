"""GPU tier: the site-fused sweep walking merged steps at either parity, chosen per pair by qk_segment_chain (csrc/qk_plan.h; QK_MERGE
unset = 2), against the oracle, against the plain chain (QK_MERGE=0) and against the merges of the fixed pairs (QK_MERGE=1).

Sets of 11 random_mps states on chains of 14 and 15 sites (n - 2 k odd and even), bonds <= 48, three bond profiles:
  flat   every bond 32 (as far as 2^k admits it): every merge admissible, the programme has to settle ties;
  dip    16 at the odd bonds, 32 at the even ones: a fixed pair (k + 2 t, k + 2 t + 1) has a dip in its middle and is refused (the merged
         tensor would cost more padded work than the two sites), a pair that starts at an odd site has the large bond in its middle and
         the dips outside and is taken;
  rising bonds 12 + 3 k (capped at 48 and by 2^k): true bonds that are no multiples of 4 or 16, tile counts that change along the chain.
Each with QK_EDGE=0, QK_EDGE=2 and QK_EDGE=4 (the planner takes edge blocks from 4 sites on, so 2 walks the whole chain like 0; 4 leaves
6 or 7 sites in the middle), in the three launch shapes (12-wave dual, 12-wave one-tile, 8-wave).  QK_FUSED=2 sends these small bonds to
the site-fused sweep.  Further: a rectangular Gram (dip x rising), launches of 1 pair and of 2 grid + 1 pairs, the same bits from two
contexts with QK_DETERMINISTIC=1, and -- with the function the device runs, compiled for the host (tools/merge_potential.py) -- that
the dip profile really takes merges at odd starts: its merged steps differ from QK_MERGE=1's.
Tolerances: the suite's TOL against the oracle, 1e-13 between two sweeps of one build."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-11
SWEEP_EPS = 1e-13
NS = 11
SHAPES = {  # shape: (switches, kernel, shape name of tools/merge_potential.py)
    "dual": ({"QK_FUSED_WGS": "1", "QK_FUSED_DUAL": "1"}, "qk_sweep_fused_dual_kernel<12, 8192, 3, {det}>", "12-wave dual (XCAP 8192)"),
    "one-tile": ({"QK_FUSED_WGS": "1", "QK_FUSED_DUAL": "0"}, "qk_sweep_fused_kernel<12, 2, 8192, 3, {det}>", "12-wave one-tile (XCAP 8192)"),
    "two-wg": ({"QK_FUSED_WGS": "2"}, "qk_sweep_fused_kernel<8, 1, 4608, 4, {det}>", "8-wave one-tile (XCAP 4608)"),
}
PROFILES = {
    "flat": lambda k: 32,
    "dip": lambda k: 16 if k % 2 else 32,
    "rising": lambda k: min(48, 12 + 3 * k),
}
_cache = {}


def _bonds(profile, n):
    return [min(2 ** min(k, n - k), PROFILES[profile](k)) for k in range(n + 1)]


def _set(profile, n, count=NS):
    """(states, K of the oracle) of a profile, made once for the module; read-only."""
    import qml_cutensornet_amd as Q
    from oracle import c_oracle

    key = (profile, n, count)
    if key not in _cache:
        rng = np.random.default_rng(1000 * n + len(profile) + count)
        xs = [Q.random_mps(n, _bonds(profile, n), rng) for _ in range(count)]
        ps = np.array([(i, j) for j in range(count) for i in range(count)], dtype=np.int32)
        v, _, _ = c_oracle.gram_pairs([m.tensors for m in xs], None, ps, 8)
        K = v.reshape(count, count)
        K.setflags(write=False)
        _cache[key] = (xs, K)
    return _cache[key]


def _potential():
    if "tool" not in _cache:
        spec = importlib.util.spec_from_file_location("merge_potential", os.path.join(ROOT, "tools", "merge_potential.py"))
        _cache["tool"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_cache["tool"])
    return _cache["tool"]


def _env(monkeypatch, shape, edge, merge, det=False):
    for k in ("QK_FUSED_WGS", "QK_FUSED_DUAL", "QK_MERGE", "QK_FUSED_SPLIT", "QK_PLAN_ORIENT", "QK_GANG"):
        monkeypatch.delenv(k, raising=False)
    for k, v in SHAPES[shape][0].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("QK_FUSED", "2")
    monkeypatch.setenv("QK_PLAN_NO_MIXED", "1")
    monkeypatch.setenv("QK_EDGE", edge)
    monkeypatch.setenv("QK_DETERMINISTIC", "1" if det else "0")
    if merge is not None:
        monkeypatch.setenv("QK_MERGE", merge)
    return SHAPES[shape][1].format(det="true" if det else "false")


def _gram(monkeypatch, shape, edge, merge, xs, det=False):
    from qml_cutensornet_amd import engine

    kernel = _env(monkeypatch, shape, edge, merge, det)
    with engine.context(0) as ctx, ctx.upload(xs) as dx:
        K = ctx.gram(dx)
        assert ctx.stats()["kernel_name"] == kernel, ctx.stats()["kernel_name"]
        plan = engine.Plan(dx.dims)
        pairs, ek, dims = plan.pairs(), plan.edge_sites, np.array(dx.dims)
        plan.close()
    return K, pairs, ek, dims


def _overlaps(monkeypatch, shape, edge, merge, xs, ys):
    from qml_cutensornet_amd import engine

    kernel = _env(monkeypatch, shape, edge, merge)
    with engine.context(0) as ctx, ctx.upload(xs) as dx, ctx.upload(ys) as dy:
        z = ctx.overlaps(dx, dy)
        st = ctx.stats()
        assert st["kernel_name"] == kernel, st["kernel_name"]
    return z, st


@pytest.mark.parametrize("edge", ["0", "2", "4"])
@pytest.mark.parametrize("n", [14, 15])
@pytest.mark.parametrize("profile", list(PROFILES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_segmented_sweep_agrees_with_the_oracle_and_both_other_rules(built, monkeypatch, shape, profile, n, edge):
    xs, K_ref = _set(profile, n)
    K, pairs, ek, dims = _gram(monkeypatch, shape, edge, None, xs)
    K0 = _gram(monkeypatch, shape, edge, "0", xs)[0]
    K1 = _gram(monkeypatch, shape, edge, "1", xs)[0]
    assert ek == (4 if edge == "4" else 0)
    tool = _potential()
    m1 = tool.merged_steps(tool.segment_pairs(dims, dims, pairs, ek, SHAPES[shape][2], 1, True)[0]).sum()
    masks2, _, steps2 = tool.segment_pairs(dims, dims, pairs, ek, SHAPES[shape][2], 3, False)
    m2 = tool.merged_steps(masks2).sum()
    odd = sum(bin(int(a) & 0xAAAAAAAAAAAAAAAA).count("1") for a in masks2[:, 0])
    print(f"{shape} {profile} n={n} QK_EDGE={edge}: max |K - oracle| {np.abs(K - K_ref).max():.2e}, |K - QK_MERGE=0| {np.abs(K - K0).max():.2e}, |K - QK_MERGE=1| {np.abs(K - K1).max():.2e}; "
          f"merged steps of {len(pairs)} pairs: QK_MERGE=1 {m1}, default {m2} ({odd} at odd starts), steps {steps2.sum()}")
    for Kc in (K, K0, K1):
        assert np.abs(Kc - K_ref).max() < TOL and np.array_equal(Kc, Kc.T)
    assert np.abs(K - K0).max() < SWEEP_EPS and np.abs(K - K1).max() < SWEEP_EPS
    if profile == "dip":  # the fixed pairs are refused, the pairs at odd starts are taken
        assert m2 != m1 and odd > 0 and m2 > m1, (m1, m2, odd)


@pytest.mark.parametrize("edge", ["0", "4"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_segmented_sweep_deterministic_mode_is_bit_identical(built, monkeypatch, shape, edge):
    xs, K_ref = _set("dip", 15)
    K1, K2 = (_gram(monkeypatch, shape, edge, None, xs, det=True)[0] for _ in range(2))
    assert np.array_equal(K1, K2)
    assert np.abs(K1 - K_ref).max() < TOL and np.array_equal(K1, K1.T)


def _rect_ref(xs, ys):
    from oracle import c_oracle

    pr = np.array([(i, j) for j in range(len(ys)) for i in range(len(xs))], dtype=np.int32)
    _, z, _ = c_oracle.gram_pairs([m.tensors for m in xs], [m.tensors for m in ys], pr, 8)
    return z.reshape(len(ys), len(xs))


@pytest.mark.parametrize("edge", ["0", "4"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_segmented_rectangular_gram(built, monkeypatch, shape, edge):
    """x set and y set differ (dip x rising, 11 x 7 states): the masks come from the bond rows of two different sets."""
    xs, ys = _set("dip", 14)[0], _set("rising", 14)[0][:7]
    if ("rect",) not in _cache:
        _cache[("rect",)] = _rect_ref(xs, ys)
    z_ref = _cache[("rect",)]
    z = _overlaps(monkeypatch, shape, edge, None, xs, ys)[0]
    z0 = _overlaps(monkeypatch, shape, edge, "0", xs, ys)[0]
    z1 = _overlaps(monkeypatch, shape, edge, "1", xs, ys)[0]
    print(f"{shape} rectangular QK_EDGE={edge}: max |z - oracle| {np.abs(z - z_ref).max():.2e}, |z - QK_MERGE=0| {np.abs(z - z0).max():.2e}, |z - QK_MERGE=1| {np.abs(z - z1).max():.2e}")
    assert z.shape == z_ref.shape and max(np.abs(zc - z_ref).max() for zc in (z, z0, z1)) < TOL
    assert np.abs(z - z0).max() < SWEEP_EPS and np.abs(z - z1).max() < SWEEP_EPS


def _factors(m):
    nx = int(m ** 0.5)
    while m % nx:
        nx -= 1
    return m // nx, nx


@pytest.mark.parametrize("wgs", [1, 2])
def test_segmented_launches_of_one_pair_and_of_two_grids_plus_one(built, monkeypatch, wgs):
    """1 pair (most workgroups get none) and 2 grid + 1 pairs (every workgroup reads the masks of several pairs, one of them a third): the
    mask of a pair is found at the pair's index in the launch's list.  Dip and flat states alternate, so neighbouring pairs differ."""
    import torch

    shape = "dual" if wgs == 1 else "two-wg"
    grid = wgs * torch.cuda.get_device_properties(0).multi_processor_count
    nx, ny = _factors(2 * grid + 1)
    dip, flat = _set("dip", 14, 24)[0], _set("flat", 14, 24)[0]
    xs = [(dip if i % 2 else flat)[(i // 2) % 24] for i in range(nx)]
    ys = [(flat if i % 3 else dip)[(i // 2) % 24] for i in range(ny)]
    for cx, cy in ((1, 1), (nx, ny)):
        z_ref = _rect_ref(xs[:cx], ys[:cy])
        z, st = _overlaps(monkeypatch, shape, "0", None, xs[:cx], ys[:cy])
        assert st["pairs"] == cx * cy and (cx * cy == 1 or st["pairs"] == 2 * st["grid"] + 1), st
        z0 = _overlaps(monkeypatch, shape, "0", "0", xs[:cx], ys[:cy])[0]
        assert z.shape == z_ref.shape and np.abs(z - z_ref).max() < TOL and np.abs(z - z0).max() < SWEEP_EPS, (cx, cy)
