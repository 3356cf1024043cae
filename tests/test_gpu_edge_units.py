"""GPU tier: the edge products of the site-fused sweep on units of one or two tiles (qk_fused.h: qkf_edge_unit, qkf_edge_prefix,
qkf_edge_suffix) and the queue pulled one pair ahead, in all three launch shapes, against the oracle and against the plain chain.

Chains of 20 sites, QK_MERGE=0.  The bonds behind the edge come from the caps of the states: the rectangular overlaps pair every x
state with every y state, so the edge products run on 16 x 16 (one tile, no partner), 16 x 48 and 48 x 16 (an odd number of column
blocks: a leftover single tile, both orientations), 32 x 80 and 128 x 128 tiles (64 tiles: several rounds; 16384 elements exceed
both LDS buffers, so prefix and suffix take the global-X path) -- as far as the depth admits them: a bond k sites from the end is at
most 2^k, so depth 4 (one group of k-steps: the steady loop never runs) has 16 x 16 only, depth 5 (two groups) up to 32 x 32, depth 7
all of them.  Tolerances: the suite's TOL against the oracle, 1e-13 between two sweeps of the same build (the bound of
test_edge_blocks_agree_with_the_plain_chain)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-11
N = 20
X_CAPS = (12, 40, 30, 128)     # padded bonds behind an edge of depth 7: 16, 48, 32, 128
Y_CAPS = (16, 48, 70, 128, 9)  # 16, 48, 80, 128, 16
SHAPES = {
    "dual": ({"QK_FUSED_WGS": "1", "QK_FUSED_DUAL": "1"}, "qk_sweep_fused_dual_kernel<12, 8192, 3, {det}>"),
    "one-tile": ({"QK_FUSED_WGS": "1", "QK_FUSED_DUAL": "0"}, "qk_sweep_fused_kernel<12, 2, 8192, 3, {det}>"),
    "two-wg": ({"QK_FUSED_WGS": "2"}, "qk_sweep_fused_kernel<8, 1, 4608, 4, {det}>"),
}


def _capped(n, cap, rng):
    import qml_cutensornet_amd as Q

    return Q.random_mps(n, [min(2 ** min(k, n - k), cap) for k in range(n + 1)], rng)


@pytest.fixture(scope="module")
def edge_sets(built):
    """The states and the oracle's results, computed once for every test of the module."""
    from oracle import restatement as R

    rng = np.random.default_rng(20)
    xs = [_capped(N, c, rng) for c in X_CAPS]
    ys = [_capped(N, c, rng) for c in Y_CAPS]
    z_ref = np.array([[R.mps_inner(x.tensors, y.tensors) for x in xs] for y in ys])
    K_ref = R.gram_from_mps([m.tensors for m in xs])
    z_ref.setflags(write=False), K_ref.setflags(write=False)
    return xs, ys, z_ref, K_ref, {}


def _sweep(monkeypatch, shape, edge, xs, ys, det=False):
    from qml_cutensornet_amd import engine

    env, name = SHAPES[shape]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("QK_MERGE", "0")
    monkeypatch.setenv("QK_EDGE", edge)
    monkeypatch.setenv("QK_DETERMINISTIC", "1" if det else "0")
    with engine.context(0) as ctx, ctx.upload(xs) as dx, ctx.upload(ys) as dy:
        K = ctx.gram(dx)
        assert ctx.stats()["kernel_name"] == name.format(det="true" if det else "false"), ctx.stats()["kernel_name"]
        z = ctx.overlaps(dx, dy)
        assert ctx.stats()["kernel_name"] == name.format(det="true" if det else "false"), ctx.stats()["kernel_name"]
    return K, z


@pytest.mark.parametrize("edge", ["4", "5", "7"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_edge_units_agree_with_the_oracle_and_the_plain_chain(edge_sets, monkeypatch, shape, edge):
    xs, ys, z_ref, K_ref, plain = edge_sets
    if shape not in plain:  # the same build without edge blocks: once per shape
        plain[shape] = _sweep(monkeypatch, shape, "0", xs, ys)
    K0, z0 = plain[shape]
    K, z = _sweep(monkeypatch, shape, edge, xs, ys)
    print(f"{shape}, QK_EDGE={edge}: max |K - oracle| {np.abs(K - K_ref).max():.2e}, |z - oracle| {np.abs(z - z_ref).max():.2e}, "
          f"|K - plain| {np.abs(K - K0).max():.2e}, |z - plain| {np.abs(z - z0).max():.2e}")
    for Kc, zc in ((K0, z0), (K, z)):
        assert np.abs(Kc - K_ref).max() < TOL and np.abs(zc - z_ref).max() < TOL
        assert np.array_equal(Kc, Kc.T)
    assert np.abs(K - K0).max() < 1e-13 and np.abs(z - z0).max() < 1e-13


@pytest.mark.parametrize("shape", list(SHAPES))
def test_edge_units_deterministic_mode_is_bit_identical(edge_sets, monkeypatch, shape):
    """QK_DETERMINISTIC=1: every wavefront leaves the share of its units in its own slot and the slots are added in wavefront order, so
    two contexts give the same bits on the same ragged set."""
    xs, ys, z_ref, K_ref, _ = edge_sets
    (K1, z1), (K2, z2) = (_sweep(monkeypatch, shape, "7", xs, ys, det=True) for _ in range(2))
    assert np.array_equal(K1, K2) and np.array_equal(z1, z2)
    assert np.abs(K1 - K_ref).max() < TOL and np.abs(z1 - z_ref).max() < TOL and np.array_equal(K1, K1.T)


def _factors(m):
    """m = nx * ny with the lists as short as they get"""
    nx = int(m ** 0.5)
    while m % nx:
        nx -= 1
    return m // nx, nx


@pytest.mark.parametrize("edge", ["4", "0"])
@pytest.mark.parametrize("wgs", [1, 2])
def test_queue_is_pulled_one_pair_ahead(built, monkeypatch, wgs, edge):
    """Launches of 1, 2 and 2 * grid + 1 pairs (grid = workgroups of a full launch): a workgroup that gets no pair, one that gets exactly
    one, and workgroups whose pull-ahead alternates an odd number of times -- with edge blocks (the pull runs beside the right edge) and
    without (it stands in front of the result's barrier).  Every overlap against the oracle."""
    import torch

    from oracle import restatement as R
    from qml_cutensornet_amd import engine

    n = 12
    grid = wgs * torch.cuda.get_device_properties(0).multi_processor_count
    nx, ny = _factors(2 * grid + 1)
    rng = np.random.default_rng(100 * wgs + int(edge))
    xs = [_capped(n, 40, rng) for _ in range(nx)]
    ys = [_capped(n, 40 if i % 2 else 20, rng) for i in range(ny)]
    monkeypatch.setenv("QK_FUSED_WGS", str(wgs))
    monkeypatch.setenv("QK_EDGE", edge)
    for cx, cy in ((1, 1), (2, 1), (nx, ny)):
        z_ref = np.array([[R.mps_inner(x.tensors, y.tensors) for x in xs[:cx]] for y in ys[:cy]])
        with engine.context(0) as ctx, ctx.upload(xs[:cx]) as dx, ctx.upload(ys[:cy]) as dy:
            z = ctx.overlaps(dx, dy)
            st = ctx.stats()
            assert "fused" in st["kernel_name"] and ("<8, 1, 4608" in st["kernel_name"]) == (wgs == 2), st["kernel_name"]
        assert z.shape == z_ref.shape and np.abs(z - z_ref).max() < TOL, (cx, cy)
