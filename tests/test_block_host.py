"""Block kernels on the host (no GPU): ``MPS.block_overlap`` -- the numpy mirror of qk_block_values_host -- against dense reduced
density matrices of states that are NOT canonical (a transposed self environment would pass on canonical ones, where every R_k is
the identity), the identities of the contract, ``engine.block_kernel``, the argument checks of ``build_block_kernel_matrices``
(raised before any device work) and the library's exports."""
import numpy as np
import pytest

import qml_cutensornet_amd as Q
from oracle import restatement as R
from qml_cutensornet_amd import engine
from test_projected_host import dense, ref_local_paulis

X_BONDS = (1, 2, 4, 8, 16, 17, 33, 70, 40, 16, 3, 2, 1)
Y_BONDS = (1, 2, 3, 5, 9, 20, 64, 65, 31, 8, 4, 2, 1)
SIDES = ("left", "right")


def gaussian_mps(bonds, rng, factor=1.0):
    """Complex Gaussian site tensors, entries scaled by 1 / sqrt(2 chi_left), not canonicalised; the state scaled by ``factor``."""
    ts = []
    for k in range(len(bonds) - 1):
        l, r = bonds[k], bonds[k + 1]
        ts.append((rng.standard_normal((l, 2, r)) + 1j * rng.standard_normal((l, 2, r))) / np.sqrt(2.0 * l))
    ts[len(ts) // 2] = ts[len(ts) // 2] * factor
    return Q.MPS(ts)


def block_sets(seed=3, nx=5, ny=4):
    """The 12-site sets of the block tests: x states on X_BONDS, y states on Y_BONDS, state 0 with the profile as given and the
    others with its interior bonds permuted per state; factors in 0.5 .. 2."""
    rng = np.random.default_rng(seed)
    out = []
    for bonds, count in ((X_BONDS, nx), (Y_BONDS, ny)):
        states = []
        for s in range(count):
            inner = list(bonds[1:-1])
            if s:
                inner = [inner[i] for i in rng.permutation(len(inner))]
            states.append(gaussian_mps([1] + inner + [1], rng, float(rng.uniform(0.5, 2.0))))
        out.append(states)
    return out


WIDE_X_BONDS = (1, 2, 4, 8, 16, 32, 64, 130, 150, 97, 48, 24, 12, 6, 3, 2, 1)
WIDE_Y_BONDS = (1, 2, 4, 8, 16, 31, 63, 113, 129, 65, 33, 17, 9, 5, 3, 2, 1)


def wide_block_sets(seed=3, nx=3, ny=2):
    """A second pair of sets, on 16 sites: bonds up to 150 and 129 (padded 160 and 144: three 64-blocks a side, unequal pads, K
    that is no multiple of 8), every state on the profile as given, factors as in ``block_sets``."""
    rng = np.random.default_rng(seed)
    return [[gaussian_mps(bonds, rng, float(rng.uniform(0.5, 2.0))) for _ in range(count)] for bonds, count in ((WIDE_X_BONDS, nx), (WIDE_Y_BONDS, ny))]


def dense_block_overlap(px, py, n, w, side):
    """tr(rho_A(x) rho_A(y)) from dense vectors (qubit 0 = most significant axis).  M[A, B] is the state as a matrix, rho_A = M M^H /
    <psi|psi>; where A is the larger half the same trace is taken as ||Mx^H My||_F^2, so no matrix exceeds 2^(n/2) rows."""
    if side == "left":
        mx, my = px.reshape(2**w, -1), py.reshape(2**w, -1)
    else:
        mx, my = px.reshape(-1, 2**w).T, py.reshape(-1, 2**w).T
    nn = float(np.vdot(px, px).real) * float(np.vdot(py, py).real)
    if mx.shape[0] <= mx.shape[1]:
        rx, ry = mx @ mx.conj().T, my @ my.conj().T
        return float(np.einsum("ab,ba->", rx, ry).real) / nn
    g = mx.conj().T @ my
    return float((np.abs(g) ** 2).sum()) / nn


@pytest.fixture(scope="module")
def pair():
    rng = np.random.default_rng(17)
    x = gaussian_mps(X_BONDS, rng, 1.7)
    y = gaussian_mps(Y_BONDS, rng, 0.6)
    return x, y, dense(x), dense(y)


# ---- the mirror against dense reduced density matrices ------------------------------------------------------------------
@pytest.mark.parametrize("side", SIDES)
def test_block_overlap_against_dense(pair, side):
    x, y, px, py = pair
    n = len(x)
    worst = 0.0
    for a, b, pa, pb in ((x, y, px, py), (x, x, px, px), (y, y, py, py)):
        for w in range(1, n + 1):
            got, ref = a.block_overlap(b, w, side), dense_block_overlap(pa, pb, n, w, side)
            worst = max(worst, abs(got - ref))
            assert 0.0 <= got <= 1.0 + 1e-12
    print(f"MPS.block_overlap vs dense reduced density matrices ({side}): max |difference| = {worst:.3e}")
    assert worst <= 1e-12


def test_block_sets_against_dense():
    xs, ys = block_sets()
    n = len(xs[0])
    assert [m.bond_dims().tolist() for m in (xs[0], ys[0])] == [list(X_BONDS), list(Y_BONDS)]
    assert xs[1].bond_dims().tolist() != list(X_BONDS) and sorted(xs[1].bond_dims().tolist()) == sorted(X_BONDS)
    x, y = xs[3], ys[2]
    px, py = dense(x), dense(y)
    for side in SIDES:
        for w in (1, 5, 7, 12):
            assert abs(x.block_overlap(y, w, side) - dense_block_overlap(px, py, n, w, side)) <= 1e-12


# ---- the identities of the contract ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", SIDES)
def test_identities(pair, side):
    x, y, px, py = pair
    n = len(x)
    nx, ny = float(np.vdot(px, px).real), float(np.vdot(py, py).real)
    # O_n is the normalised fidelity
    assert abs(x.block_overlap(y, n, side) - abs(np.vdot(px, py)) ** 2 / (nx * ny)) <= 1e-12
    assert abs(x.block_overlap(x, n, side) - 1.0) <= 1e-12
    # O_1 from the Bloch vectors of the end qubit
    q = 0 if side == "left" else n - 1
    fx, fy = ref_local_paulis(x.tensors)[0], ref_local_paulis(y.tensors)[0]
    assert abs(x.block_overlap(y, 1, side) - 0.5 * (1.0 + float(fx[q] @ fy[q]))) <= 1e-12
    # S_w is the purity of the cut: the sum of the squared Schmidt weights
    for m in (x, y):
        spectra = m.bond_spectra()
        for w in range(1, n):
            bond = w if side == "left" else n - w
            assert abs(m.block_overlap(m, w, side) - float((spectra[bond - 1] ** 2).sum())) <= 1e-12
    # O_w(x, y) = O_w(y, x), and Cauchy-Schwarz
    for w in range(1, n + 1):
        o = x.block_overlap(y, w, side)
        assert abs(o - y.block_overlap(x, w, side)) <= 1e-14
        assert o <= np.sqrt(x.block_overlap(x, w, side) * y.block_overlap(y, w, side)) + 1e-14


def test_block_overlap_argument_errors(pair):
    x, y, _, _ = pair
    for bad in (0, 13, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="width"):
            x.block_overlap(y, bad)
    with pytest.raises(ValueError, match="side"):
        x.block_overlap(y, 3, side="middle")
    with pytest.raises(ValueError, match="same number of sites"):
        x.block_overlap(Q.random_mps(3, [1, 2, 2, 1], np.random.default_rng(0)), 1)


# ---- states of the ansatz against the state-vector oracle ---------------------------------------------------------------
def test_ansatz_states_against_statevector():
    n, reps = 8, 2
    edges = Q.entanglement_graph(n, 2)
    ans = Q.KernelStateAnsatz(n, reps, 1.0, edges)
    X = R.synthetic_features(3, n, 21)
    states = [Q.simulate(ans.circuit_for_data(x), 1 - 1e-16) for x in X]
    vecs = [R.statevector(n, R.ansatz_gates(x, reps, 1.0, edges)) for x in X]
    worst = 0.0
    for side in SIDES:
        for i in range(3):
            for j in range(i, 3):
                for w in range(1, n + 1):
                    worst = max(worst, abs(states[i].block_overlap(states[j], w, side) - dense_block_overlap(vecs[i], vecs[j], n, w, side)))
    print(f"block overlaps of built states vs the state-vector oracle: max |difference| = {worst:.3e}")
    assert worst <= 1e-10


# ---- engine.block_kernel ------------------------------------------------------------------------------------------------------
def _overlap_tables(pair_states, widths, side="left"):
    xs, ys = pair_states
    O = np.array([[[x.block_overlap(y, w, side) for x in xs] for y in ys] for w in widths])
    Sx = np.array([[x.block_overlap(x, w, side) for x in xs] for w in widths])
    Sy = np.array([[y.block_overlap(y, w, side) for y in ys] for w in widths])
    return O, Sx, Sy


def test_block_kernel_forms():
    rng = np.random.default_rng(5)
    xs = [gaussian_mps((1, 2, 4, 3, 2, 1), rng, f) for f in (0.5, 1.0, 2.0)]
    ys = [gaussian_mps((1, 2, 3, 4, 2, 1), rng, f) for f in (0.7, 1.3)]
    widths = (1, 3, 5)
    O, Sx, Sy = _overlap_tables((xs, ys), widths)
    assert np.array_equal(engine.block_kernel(O, Sx, Sy, form="overlap"), O)
    Kn = engine.block_kernel(O, Sx, Sy, form="normalized")
    Kr = engine.block_kernel(O, Sx, Sy, form="rbf", gamma=0.7)
    assert np.array_equal(engine.block_kernel(O, Sx, Sy), engine.block_kernel(O, Sx, Sy, form="rbf", gamma=1.0))
    for wi in range(len(widths)):
        for j in range(2):
            for i in range(3):
                assert abs(Kn[wi, j, i] - O[wi, j, i] / np.sqrt(Sx[wi, i] * Sy[wi, j])) <= 1e-15
                assert abs(Kr[wi, j, i] - np.exp(-0.7 * (Sx[wi, i] + Sy[wi, j] - 2 * O[wi, j, i]))) <= 1e-15
    assert np.all(Kn <= 1.0 + 1e-12) and np.all(Kr <= 1.0 + 1e-12)
    # the rbf form is the Frobenius distance of the reduced density matrices
    px, py = dense(xs[0]), dense(ys[1])
    mx, my = px.reshape(8, -1), py.reshape(8, -1)
    d = mx @ mx.conj().T / np.vdot(px, px).real - my @ my.conj().T / np.vdot(py, py).real
    assert abs(Kr[1, 1, 0] - np.exp(-0.7 * float((np.abs(d) ** 2).sum()))) <= 1e-13
    # one width at a time is the same
    assert np.array_equal(engine.block_kernel(O[1], Sx[1], Sy[1], form="normalized"), Kn[1])


def test_block_kernel_symmetric_is_exact():
    rng = np.random.default_rng(6)
    xs = [gaussian_mps((1, 2, 4, 3, 2, 1), rng, f) for f in (0.5, 1.0, 2.0, 1.1)]
    O, Sx, _ = _overlap_tables((xs, xs), (2, 4))
    O = O + 1e-17 * rng.standard_normal(O.shape)  # rounding noise between (i, j) and (j, i) must not show
    for form in ("overlap", "normalized", "rbf"):
        K = engine.block_kernel(O, Sx, form=form)
        assert np.array_equal(K, np.swapaxes(K, -1, -2))
        if form != "overlap":
            assert np.all(K[:, np.arange(4), np.arange(4)] == 1.0)
        assert np.abs(K - engine.block_kernel(O, Sx, Sx, form=form)).max() <= 1e-15  # the rectangular call on the same numbers


def test_block_kernel_argument_errors():
    O, Sx, Sy = np.full((2, 3, 4), 0.5), np.ones((2, 4)), np.ones((2, 3))
    with pytest.raises(ValueError, match="form"):
        engine.block_kernel(O, Sx, Sy, form="gaussian")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="gamma"):
            engine.block_kernel(O, Sx, Sy, gamma=bad)
    with pytest.raises(ValueError, match="shape"):
        engine.block_kernel(O, Sy, Sx)
    with pytest.raises(ValueError, match="shape"):
        engine.block_kernel(O, Sx)  # Y is X needs a square O
    with pytest.raises(ValueError, match="shape"):
        engine.block_kernel(O[0, 0], Sx[0], Sy[0])


# ---- the public surface without a device ----------------------------------------------------------------------------------
@pytest.mark.parametrize(
    "kwargs,match",
    [
        ({"Y": np.zeros((5, 4)), "truncation_error": 1e-16}, "X must not be smaller than Y"),
        ({"truncation_error": None}, "truncation error"),
        ({"truncation_error": 1e-16, "widths": ()}, "widths"),
        ({"truncation_error": 1e-16, "widths": (0, 2)}, "widths"),
        ({"truncation_error": 1e-16, "widths": (1, 5)}, "widths"),
        ({"truncation_error": 1e-16, "widths": (2, 2)}, "widths"),
        ({"truncation_error": 1e-16, "widths": (3, 1)}, "widths"),
        ({"truncation_error": 1e-16, "widths": (1.0, 2)}, "widths"),
        ({"truncation_error": 1e-16, "side": "middle"}, "side"),
        ({"truncation_error": 1e-16, "form": "gaussian"}, "form"),
        ({"truncation_error": 1e-16, "block_gamma": 0.0}, "block_gamma"),
        ({"truncation_error": 1e-16, "block_gamma": float("nan")}, "block_gamma"),
    ],
)
def test_build_block_kernel_matrices_argument_errors(monkeypatch, kwargs, match):
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend import kernel_state_ansatz as K

    def no_device(*a, **k):
        raise AssertionError("device work before the argument checks")

    monkeypatch.setattr(engine, "device_count", no_device)
    monkeypatch.setattr(engine, "default_context", no_device)
    ans = Q.KernelStateAnsatz(4, 1, 1.0, Q.entanglement_graph(4, 1))
    with pytest.raises(ValueError, match=match):
        K.build_block_kernel_matrices(SingleComm(), ans, np.zeros((3, 4)), **kwargs)


def test_library_exports_block_entry_points(built):
    L = engine.lib()
    for name in ("qk_block_values_host", "qk_block_self_host"):
        assert name in engine.EXPORTED_SYMBOLS
        assert hasattr(L, name)
