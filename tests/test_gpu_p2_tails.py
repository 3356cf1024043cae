"""GPU tier: phase 2 of the site-fused sweep (qk_fused.h: qkf_p2_block, qkf_p2_item, qkf_p2_dual_turn) -- the plain forms take the 3M
product's recombination on the accumulators (k1 = sum (tr + ti) Ar starts the chains of re and im), the DET forms keep the ordered
product -- in all three launch shapes, against the oracle and against a second sweep of the same build.

Chains of 20 sites.  The caps of the x states give row blocks of A whose last one holds 1, 1, 2, 3, 2 and 1 k-steps below the true bond
(bonds 3, 17, 22, 27, 40, 100: the instantiations with kmax < 4, a block of ONE k-step being the smallest case), a single column
block of X' (bond 3 and the ends of every chain: only the block that reloads the next stream runs) and, at 100 x 100 (112 x 112
padded = 12544 elements, more than either LDS buffer), the global-X path with several strips.  The y caps give an odd number of column
blocks of B (a leftover single tile and the halved last round of the dual kernel), in-place and ping-pong steps.  Every case runs once
with QK_EDGE=0 QK_MERGE=0 (X_0 = 1, plain sites, the result read from LDS) and once with the defaults (edge prefix and suffix through
LDS, merged steps with four physical indices).  Tolerances: the suite's TOL against the oracle, 1e-13 between two sweeps of one build
(the bound of test_edge_blocks_agree_with_the_plain_chain)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-11
N = 20
X_CAPS = (3, 17, 22, 27, 40, 100)
Y_CAPS = (16, 48, 70, 128, 9)
SHAPES = {
    "dual": ({"QK_FUSED_WGS": "1", "QK_FUSED_DUAL": "1"}, "qk_sweep_fused_dual_kernel<12, 8192, 3, {det}>"),
    "one-tile": ({"QK_FUSED_WGS": "1", "QK_FUSED_DUAL": "0"}, "qk_sweep_fused_kernel<12, 2, 8192, 3, {det}>"),
    "two-wg": ({"QK_FUSED_WGS": "2"}, "qk_sweep_fused_kernel<8, 1, 4608, 4, {det}>"),
}


def _capped(n, cap, rng):
    import qml_cutensornet_amd as Q

    return Q.random_mps(n, [min(2 ** min(k, n - k), cap) for k in range(n + 1)], rng)


@pytest.fixture(scope="module")
def tail_sets(built):
    """The states and the oracle's results, computed once for every test of the module."""
    from oracle import restatement as R

    rng = np.random.default_rng(27)
    xs = [_capped(N, c, rng) for c in X_CAPS]
    ys = [_capped(N, c, rng) for c in Y_CAPS]
    z_ref = np.array([[R.mps_inner(x.tensors, y.tensors) for x in xs] for y in ys])
    K_ref = R.gram_from_mps([m.tensors for m in xs])
    z_ref.setflags(write=False), K_ref.setflags(write=False)
    return xs, ys, z_ref, K_ref


def _sweep(monkeypatch, shape, plain_chain, xs, ys, det):
    from qml_cutensornet_amd import engine

    env, name = SHAPES[shape]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for k in ("QK_EDGE", "QK_MERGE"):
        if plain_chain:
            monkeypatch.setenv(k, "0")
        else:
            monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("QK_DETERMINISTIC", "1" if det else "0")
    with engine.context(0) as ctx, ctx.upload(xs) as dx, ctx.upload(ys) as dy:
        K = ctx.gram(dx)
        assert ctx.stats()["kernel_name"] == name.format(det="true" if det else "false"), ctx.stats()["kernel_name"]
        z = ctx.overlaps(dx, dy)
        assert ctx.stats()["kernel_name"] == name.format(det="true" if det else "false"), ctx.stats()["kernel_name"]
    return K, z


@pytest.mark.parametrize("det", [False, True], ids=["plain", "det"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_p2_tails_agree_with_the_oracle_and_between_chains(tail_sets, monkeypatch, shape, det):
    xs, ys, z_ref, K_ref = tail_sets
    K0, z0 = _sweep(monkeypatch, shape, True, xs, ys, det)
    K, z = _sweep(monkeypatch, shape, False, xs, ys, det)
    print(f"{shape}, det {det}: max |K - oracle| {np.abs(K - K_ref).max():.2e} / {np.abs(K0 - K_ref).max():.2e}, |z - oracle| {np.abs(z - z_ref).max():.2e} / "
          f"{np.abs(z0 - z_ref).max():.2e}, |K - plain chain| {np.abs(K - K0).max():.2e}, |z - plain chain| {np.abs(z - z0).max():.2e}")
    for Kc, zc in ((K0, z0), (K, z)):
        assert np.abs(Kc - K_ref).max() < TOL and np.abs(zc - z_ref).max() < TOL
        assert np.array_equal(Kc, Kc.T)
    assert np.abs(K - K0).max() < 1e-13 and np.abs(z - z0).max() < 1e-13
    if det:  # the ordered forms: the same bits from a second context, with and without edge blocks and merged steps
        for plain_chain, (Ka, za) in ((True, (K0, z0)), (False, (K, z))):
            Kb, zb = _sweep(monkeypatch, shape, plain_chain, xs, ys, True)
            assert np.array_equal(Ka, Kb) and np.array_equal(za, zb)
