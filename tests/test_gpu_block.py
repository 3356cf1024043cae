"""Block kernels on the MI355X: qk_block_values_host / qk_block_self_host against the host mirror ``MPS.block_overlap`` on identical
tensors (12-site sets whose bonds cross the 16 padding and the 64-block edge, with unequal pad_x / pad_y and K that is no multiple
of the K-tile; 16-site sets with bonds up to 150 against 129: three 64-blocks a side), the identities of the contract on the device,
the bit guarantees (a pair alone, a width subset, the batches cut by QK_BLOCK_BATCH, two runs, the plans of two ranks), short
chains, the rejections, and build_block_kernel_matrices end to end.

Bounds: 1e-11 absolute for HIP against the host on identical tensors (the values are <= 1), 1e-9 for a builder against another
builder or the state-vector oracle."""
import numpy as np
import pytest

import qml_cutensornet_amd as Q
from oracle import restatement as R
from qml_cutensornet_amd import engine
from qml_cutensornet_amd.dist import SingleComm, assemble_gram
from test_block_host import SIDES, block_sets, dense_block_overlap, gaussian_mps, wide_block_sets

pytestmark = pytest.mark.gpu
N = 12
ALL = list(range(1, N + 1))


@pytest.fixture(scope="module")
def sets():
    return block_sets()


@pytest.fixture(scope="module")
def host_ref(sets):
    """The host mirror, once for the module: per side O (12, ny, nx), the symmetric O of the x states, Sx, Sy."""
    xs, ys = sets
    ref = {}
    for side in SIDES:
        O = np.array([[[x.block_overlap(y, w, side) for x in xs] for y in ys] for w in ALL])
        Oxx = np.zeros((N, len(xs), len(xs)))
        for i in range(len(xs)):
            for j in range(i, len(xs)):
                for w in ALL:
                    Oxx[w - 1, j, i] = Oxx[w - 1, i, j] = xs[i].block_overlap(xs[j], w, side)
        Sy = np.array([[y.block_overlap(y, w, side) for y in ys] for w in ALL])
        ref[side] = (O, Oxx, Oxx[:, np.arange(len(xs)), np.arange(len(xs))].copy(), Sy)
    return ref


@pytest.fixture(scope="module")
def dev(gpu_ctx, sets):
    """The two sets on the device and, per side, the results of the full calls (all widths)."""
    xs, ys = sets
    with gpu_ctx.upload(xs) as dx, gpu_ctx.upload(ys) as dy:
        full = {side: (gpu_ctx.block_overlaps(dx, dy, None, side), gpu_ctx.block_overlaps(dx, None, None, side)) for side in SIDES}
        yield dx, dy, full


# ---- 1. against the host mirror on identical tensors ------------------------------------------------------------------------
@pytest.mark.parametrize("side", SIDES)
def test_rectangular_against_host(dev, host_ref, side):
    (O, Sx, Sy), _ = dev[2][side]
    rO, _, rSx, rSy = host_ref[side]
    assert O.shape == (N, 4, 5) and Sx.shape == (N, 5) and Sy.shape == (N, 4) and O.dtype == np.float64
    errs = [float(np.abs(a - b).max()) for a, b in ((O, rO), (Sx, rSx), (Sy, rSy))]
    print(f"block overlaps vs MPS.block_overlap ({side}, rectangular): max |dO| = {errs[0]:.3e}, |dSx| = {errs[1]:.3e}, |dSy| = {errs[2]:.3e}")
    assert max(errs) <= 1e-11
    assert np.all(O >= -1e-11) and np.all(O <= np.sqrt(Sx[:, None, :] * Sy[:, :, None]) + 1e-11)


@pytest.mark.parametrize("side", SIDES)
def test_symmetric_against_host(gpu_ctx, dev, host_ref, side):
    dx = dev[0]
    _, (O, Sx, Sy) = dev[2][side]
    _, rOxx, rSx, _ = host_ref[side]
    assert O.shape == (N, 5, 5) and Sy is Sx
    err = float(np.abs(O - rOxx).max())
    print(f"block overlaps vs MPS.block_overlap ({side}, symmetric): max |dO| = {err:.3e}")
    assert err <= 1e-11
    assert np.array_equal(O, np.swapaxes(O, 1, 2))
    # the diagonal of a symmetric call is block_self, bit for bit
    S = gpu_ctx.block_self(dx, None, side)
    assert np.array_equal(O[:, np.arange(5), np.arange(5)], S) and np.array_equal(Sx, S)


@pytest.fixture(scope="module")
def wide(gpu_ctx):
    """The 16-site sets of ``wide_block_sets`` (three 64-blocks a side), per side: the device's rectangular and symmetric results
    over all 16 widths, block_self, and the host mirror of each, computed once."""
    xs, ys = wide_block_sets()
    widths = list(range(1, 17))
    out = {}
    with gpu_ctx.upload(xs) as dx, gpu_ctx.upload(ys) as dy:
        assert int(np.asarray(dx.dims).max()) == 150 and int(np.asarray(dy.dims).max()) == 129
        for side in SIDES:
            rO = np.array([[[x.block_overlap(y, w, side) for x in xs] for y in ys] for w in widths])
            rOxx = np.zeros((16, len(xs), len(xs)))
            for i in range(len(xs)):
                for j in range(i, len(xs)):
                    for w in widths:
                        rOxx[w - 1, j, i] = rOxx[w - 1, i, j] = xs[i].block_overlap(xs[j], w, side)
            rSy = np.array([[y.block_overlap(y, w, side) for y in ys] for w in widths])
            out[side] = (gpu_ctx.block_overlaps(dx, dy, None, side), gpu_ctx.block_overlaps(dx, None, None, side), gpu_ctx.block_self(dx, None, side),
                         (rO, rOxx, rSy))
    return out


@pytest.mark.parametrize("side", SIDES)
def test_three_blocks_a_side_against_host(wide, side):
    """Bonds up to 150 against 129 on 16 sites: three 64-blocks a side where ``block_sets`` has two, pads of 160 against 144, K =
    130, 97, 113, 129.  Measured on the MI355X: max |dO| = 2.8e-16 (rectangular) and 1.3e-15 (symmetric, purities included), the values from
    1.4e-7 to 0.66, so the absolute bound still resolves the smallest."""
    (O, Sx, Sy), (Oxx, Sxx, _), S, (rO, rOxx, rSy) = wide[side]
    assert O.shape == (16, 2, 3) and Oxx.shape == (16, 3, 3)
    rSx = rOxx[:, np.arange(3), np.arange(3)]
    errs = [float(np.abs(a - b).max()) for a, b in ((O, rO), (Sx, rSx), (Sy, rSy), (Oxx, rOxx))]
    print(f"block overlaps vs MPS.block_overlap ({side}, three blocks a side): max |dO| = {errs[0]:.3e}, |dSx| = {errs[1]:.3e}, |dSy| = {errs[2]:.3e}, "
          f"symmetric |dO| = {errs[3]:.3e}; reference values from {min(rO.min(), rOxx.min()):.2e} to {rO.max():.2e}")
    assert max(errs) <= 1e-11
    assert min(rO.min(), rOxx.min()) >= 1e-7  # a condition on the inputs: the absolute bound is at most 1e-4 of the smallest value
    assert np.array_equal(Oxx, np.swapaxes(Oxx, 1, 2))
    # the diagonal of a symmetric call is block_self, bit for bit
    assert np.array_equal(Oxx[:, np.arange(3), np.arange(3)], S) and np.array_equal(Sxx, S)


# ---- 2. the identities on the device -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", SIDES)
def test_identities_on_device(gpu_ctx, dev, side):
    dx, dy, full = dev
    (O, Sx, Sy), _ = full[side]
    Fx, nx = gpu_ctx.local_paulis(dx, norms=True)
    Fy, ny = gpu_ctx.local_paulis(dy, norms=True)
    # O_n is the fidelity Gram divided by the norms
    G = gpu_ctx.gram(dx, dy) / (nx[None, :] * ny[:, None])
    e_n = float(np.abs(O[N - 1] - G).max())
    # O_1 from the Bloch vectors of the end qubit
    q = 0 if side == "left" else N - 1
    e_1 = float(np.abs(O[0] - 0.5 * (1.0 + Fy[:, q] @ Fx[:, q].T)).max())
    # S_w is the purity of the cut, S_n = 1
    e_s = 0.0
    for S, d in ((Sx, dx), (Sy, dy)):
        pur = gpu_ctx.bond_purities(d)
        for w in range(1, N):
            e_s = max(e_s, float(np.abs(S[w - 1] - pur[:, (w if side == "left" else N - w) - 1]).max()))
        e_s = max(e_s, float(np.abs(S[N - 1] - 1.0).max()))
    print(f"identities on the device ({side}): |O_n - gram/norms| = {e_n:.3e}, |O_1 - Bloch| = {e_1:.3e}, |S_w - purity| = {e_s:.3e}")
    assert e_n <= 1e-11 and e_1 <= 1e-11 and e_s <= 1e-11
    # the norms block_self returns are the bits of local_paulis
    _, nrm = gpu_ctx.block_self(dx, (1,), side, norms=True)
    assert np.array_equal(nrm, nx)


# ---- 3. bits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", SIDES)
def test_bits(gpu_ctx, sets, dev, side, monkeypatch):
    xs, ys = sets
    dx, dy, full = dev
    (O, Sx, Sy), (Oxx, _, _) = full[side]
    monkeypatch.delenv("QK_BLOCK_BATCH", raising=False)
    # a second run
    O2, Sx2, Sy2 = gpu_ctx.block_overlaps(dx, dy, None, side)
    assert np.array_equal(O2, O) and np.array_equal(Sx2, Sx) and np.array_equal(Sy2, Sy)
    # one pair alone, in sets of one state
    with gpu_ctx.upload([xs[2]]) as ax, gpu_ctx.upload([ys[1]]) as ay:
        O1, _, _ = gpu_ctx.block_overlaps(ax, ay, None, side)
    assert np.array_equal(O1[:, 0, 0], O[:, 1, 2])
    # a width subset against all widths
    sub = [3, 7, 12]
    Os, Sxs, _ = gpu_ctx.block_overlaps(dx, dy, sub, side)
    assert np.array_equal(Os, O[[w - 1 for w in sub]]) and np.array_equal(Sxs, Sx[[w - 1 for w in sub]])
    assert np.array_equal(gpu_ctx.block_overlaps(dx, None, [5], side)[0][0], Oxx[4])
    # the cut into pair batches
    for cap in ("1", "3"):
        monkeypatch.setenv("QK_BLOCK_BATCH", cap)
        Ob, Sxb, Syb = gpu_ctx.block_overlaps(dx, dy, None, side)
        assert np.array_equal(Ob, O) and np.array_equal(Sxb, Sx) and np.array_equal(Syb, Sy)
        assert np.array_equal(gpu_ctx.block_overlaps(dx, None, None, side)[0], Oxx)
    monkeypatch.setenv("QK_BLOCK_BATCH", "0")
    with pytest.raises(engine.QkError, match="QK_BLOCK_BATCH"):
        gpu_ctx.block_self(dx, (1,), side)


# ---- 4. plans ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symmetric", [False, True], ids=["rectangular", "symmetric"])
def test_two_rank_plans_equal_one(gpu_ctx, dev, symmetric):
    dx, dy, full = dev
    ys = None if symmetric else dy
    want = full["left"][1 if symmetric else 0][0]
    ny = len(dx) if symmetric else len(dy)
    pairs, vals = [], []
    for r in range(2):
        plan = engine.Plan(dx.dims, None if symmetric else dy.dims, 2, r, orient=False)
        pairs.append(plan.pairs())
        vals.append(gpu_ctx.block_values_host(dx, ys, plan, ALL, "left"))
        assert vals[-1].shape == (N, plan.num_pairs)
        plan.close()
    assert sum(len(p) for p in pairs) == (15 if symmetric else 20)
    for wi in range(N):
        K = assemble_gram(ny, len(dx), pairs, [v[wi] for v in vals], symmetric)
        assert np.array_equal(K, want[wi])


# ---- 5. short chains ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bonds_x,bonds_y", [((1, 1), (1, 1)), ((1, 2, 1), (1, 2, 1)), ((1, 2, 1), (1, 1, 1)), ((1, 1, 1, 1, 1, 1), (1, 2, 4, 4, 2, 1))],
                         ids=["one-site", "two-sites", "two-sites-bond1", "every-bond-1"])
def test_short_chains(gpu_ctx, bonds_x, bonds_y):
    rng = np.random.default_rng(12)
    xs = [gaussian_mps(bonds_x, rng, f) for f in (0.6, 1.5)]
    ys = [gaussian_mps(bonds_y, rng, f) for f in (1.2, 0.8, 1.0)]
    n = len(bonds_x) - 1
    for side in SIDES:
        with gpu_ctx.upload(xs) as dx, gpu_ctx.upload(ys) as dy:
            O, Sx, Sy = gpu_ctx.block_overlaps(dx, dy, None, side)
        assert O.shape == (n, 3, 2)
        ref = np.array([[[x.block_overlap(y, w, side) for x in xs] for y in ys] for w in range(1, n + 1)])
        assert np.abs(O - ref).max() <= 1e-11
        assert np.abs(Sx - np.array([[x.block_overlap(x, w, side) for x in xs] for w in range(1, n + 1)])).max() <= 1e-11
        if max(bonds_x) == 1:  # a product state: every cut is pure
            assert np.abs(Sx - 1.0).max() <= 1e-11


# ---- 6. the rejections -------------------------------------------------------------------------------------------------------------
def _raw_values(ctx, xset, yset, plan, side, n_widths, widths, out):
    rc = engine.lib().qk_block_values_host(ctx, xset, yset, plan, side, n_widths, widths, out)
    engine._check(rc, "qk_block_values_host")


def test_argument_errors(gpu_ctx, sets, dev):
    xs, ys = sets
    dx, dy, _ = dev
    plan = engine.Plan(dx.dims, dy.dims)
    w = np.array([1, 2], dtype=np.int32)
    out = np.zeros((2, plan.num_pairs))
    ok = (gpu_ctx.handle, dx.handle, dy.handle, plan.handle, 0, 2, w.ctypes.data, out.ctypes.data)
    for k in (0, 1, 3, 6, 7):  # a null ctx, xset, plan, widths, values_host (yset may be null)
        args = list(ok)
        args[k] = None
        with pytest.raises(engine.QkError, match="null"):
            _raw_values(*args)
    so = np.zeros((2, len(dx)))
    L = engine.lib()
    for args in ((None, dx.handle, 0, 2, w.ctypes.data, so.ctypes.data, None), (gpu_ctx.handle, None, 0, 2, w.ctypes.data, so.ctypes.data, None),
                 (gpu_ctx.handle, dx.handle, 0, 2, None, so.ctypes.data, None), (gpu_ctx.handle, dx.handle, 0, 2, w.ctypes.data, None, None)):
        with pytest.raises(engine.QkError, match="null"):
            engine._check(L.qk_block_self_host(*args), "qk_block_self_host")
    # a set of another context
    other = engine.Context(0)
    try:
        with other.upload(ys) as oy:
            with pytest.raises(engine.QkError, match="another context"):
                gpu_ctx.block_values_host(dx, oy, plan, [1, 2])
            with pytest.raises(engine.QkError, match="another context"):
                gpu_ctx.block_self(oy, [1])
    finally:
        other.close()
    # a complex64 set
    with dx.to_f32() as fx:
        with pytest.raises(engine.QkError, match="complex64"):
            gpu_ctx.block_values_host(fx, dy, plan, [1, 2])
        with pytest.raises(engine.QkError, match="complex64"):
            gpu_ctx.block_values_host(dx, fx, plan, [1, 2])
        with pytest.raises(engine.QkError, match="complex64"):
            gpu_ctx.block_self(fx, [1])
    # two sets whose numbers of sites differ
    with gpu_ctx.upload([gaussian_mps((1, 2, 2, 1), np.random.default_rng(0))] * 4) as short:
        with pytest.raises(engine.QkError, match="site counts differ"):
            gpu_ctx.block_values_host(dx, short, plan, [1, 2])
    # a plan whose pair indices exceed the sets
    with gpu_ctx.upload(xs[:3]) as three:
        with pytest.raises(engine.QkError, match="pair"):
            gpu_ctx.block_values_host(three, dy, plan, [1, 2])
        with pytest.raises(engine.QkError, match="pair"):
            gpu_ctx.block_values_host(dy, three, plan, [1, 2])
    # side, n_widths, widths
    for side in (2, -1):
        with pytest.raises(engine.QkError, match="side"):
            gpu_ctx.block_values_host(dx, dy, plan, [1, 2], side)
        with pytest.raises(engine.QkError, match="side"):
            gpu_ctx.block_self(dx, [1, 2], side)
    with pytest.raises(engine.QkError, match="n_widths"):
        gpu_ctx.block_values_host(dx, dy, plan, [])
    with pytest.raises(engine.QkError, match="n_widths"):
        gpu_ctx.block_self(dx, [])
    for bad in ([0, 1], [1, 13], [2, 2], [3, 1], [-1]):
        with pytest.raises(engine.QkError, match="widths"):
            gpu_ctx.block_values_host(dx, dy, plan, bad)
        with pytest.raises(engine.QkError, match="widths"):
            gpu_ctx.block_self(dx, bad)
    plan.close()
    with pytest.raises(ValueError, match="side"):
        gpu_ctx.block_self(dx, [1], "middle")
    with pytest.raises(ValueError, match="widths"):
        gpu_ctx.block_self(dx, [1.5])
    # the Gram statistics are not touched, and the scratch goes back
    before = gpu_ctx.stats()
    gpu_ctx.block_self(dx, [1, 12])
    assert gpu_ctx.stats() == before
    gpu_ctx.trim()


# ---- 7. end to end -----------------------------------------------------------------------------------------------------------------
def test_build_block_kernel_matrices(built):
    from qml_cutensornet_amd.gpu_backend import kernel_state_ansatz as K

    n, reps = 8, 2
    edges = Q.entanglement_graph(n, 2)
    ans = Q.KernelStateAnsatz(n, reps, 1.0, edges)
    X, Y = R.synthetic_features(6, n, 31), R.synthetic_features(4, n, 32)
    widths = (1, 4, 8)
    vx = [R.statevector(n, R.ansatz_gates(x, reps, 1.0, edges)) for x in X]
    vy = [R.statevector(n, R.ansatz_gates(y, reps, 1.0, edges)) for y in Y]
    for side in SIDES:
        rO = np.array([[[dense_block_overlap(a, b, n, w, side) for a in vx] for b in vy] for w in widths])
        rSx = np.array([[dense_block_overlap(a, a, n, w, side) for a in vx] for w in widths])
        rSy = np.array([[dense_block_overlap(b, b, n, w, side) for b in vy] for w in widths])
        for form, gamma in (("rbf", 0.8), ("normalized", None)):
            out = K.build_block_kernel_matrices(SingleComm(), ans, X, Y, widths=widths, side=side, form=form, block_gamma=gamma, truncation_error=1e-16)
            assert out["widths"] == list(widths) and out["self_x"].shape == (3, 6) and out["self_y"].shape == (3, 4)
            rK = engine.block_kernel(rO, rSx, rSy, form=form, gamma=gamma)
            for wi, w in enumerate(widths):
                assert out["K"][w].shape == (4, 6)
                assert np.abs(out["overlap"][w] - rO[wi]).max() <= 1e-9
                assert np.abs(out["K"][w] - rK[wi]).max() <= 1e-9
            assert np.abs(out["self_x"] - rSx).max() <= 1e-9 and np.abs(out["self_y"] - rSy).max() <= 1e-9
    # width n, "overlap", is the fidelity kernel
    out = K.build_block_kernel_matrices(SingleComm(), ans, X, Y, widths=(8,), form="overlap", truncation_error=1e-16)
    Kf = K.build_kernel_matrix(SingleComm(), ans, X, Y, truncation_error=1e-16)
    assert np.abs(out["K"][8] - Kf).max() <= 1e-9
    # a symmetric call
    sym = K.build_block_kernel_matrices(SingleComm(), ans, X, widths=(2, 8), truncation_error=1e-16)
    for w in (2, 8):
        assert np.array_equal(sym["K"][w], sym["K"][w].T) and np.all(np.diag(sym["K"][w]) == 1.0)
    assert sym["self_y"] is sym["self_x"]
    assert np.abs(sym["overlap"][2] - np.array([[dense_block_overlap(a, b, n, 2, "left") for a in vx] for b in vx])).max() <= 1e-9
