"""Applying an MPO to a state on the host (no GPU): ``MPS.apply_mpo`` -- the numpy mirror of qk_mps_set_apply_mpo and the oracle of
tests/test_gpu_apply.py -- against ``to_dense(mpo) @ vec(psi)`` on at most 8 qubits, composition against ``B @ A``, the parity
projectors (``P P psi = P psi``, both signs, subsets of the qubits), ``mpo_two_qubit_gate`` against ``simulate`` of the same circuit
with the SWAP-routed ``Unitary2q`` appended (adjacent, distant and reversed qubits, CX with bond 2), the index convention (u-major
rows, v-major columns) on a hand-made 2-site case, and the constructor errors.

Tolerances: the states have unit norm and the random MPOs have every matricised tensor at spectral norm 1
(tests/test_mpo_host.py), so every vector element is of magnitude <= 1 and 1e-12 is the project's bound for unit-scale values."""
import numpy as np
import pytest

import qml_cutensornet_amd as Q
from helpers import scrambled
from qml_cutensornet_amd import engine
from test_matrix_gates_host import NAMED, brickwork, features, from_gates, haar
from test_mpo_host import heisenberg_terms, random_dense_mpo
from test_projected_host import dense


def unit_mps(n, profile, rng):
    m = scrambled(Q.random_mps(n, profile, rng), rng)
    nrm = np.linalg.norm(dense(m))
    return Q.MPS([t / nrm if k == 0 else t for k, t in enumerate(m.tensors)])


CASES = {  # name: (n, state profile, MPO bonds)
    "n8": (8, [1, 2, 4, 7, 9, 8, 4, 2, 1], [1, 3, 2, 5, 4, 2, 3, 2, 1]),
    "n5 odd": (5, [1, 2, 3, 3, 2, 1], [1, 2, 3, 5, 3, 1]),
    "n1": (1, [1, 1], [1, 1]),
    "n6 bond 1": (6, [1, 2, 4, 5, 4, 2, 1], [1, 1, 1, 1, 1, 1, 1]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_mirror_against_the_dense_product(name):
    n, prof, bonds = CASES[name]
    rng = np.random.default_rng(41)
    psi, O = unit_mps(n, prof, rng), random_dense_mpo(rng, bonds)
    assert max(np.abs(t).max() for t in O.tensors) <= 1.0 and abs(np.linalg.norm(dense(psi)) - 1) < 1e-13
    out = psi.apply_mpo(O)
    assert list(out.bond_dims()) == [w * c for w, c in zip(bonds, prof)]
    err = np.abs(dense(out) - O.to_dense() @ dense(psi)).max()
    print(f"{name}: max |mirror - dense| = {err:.3e}")
    assert err <= 1e-12
    assert all(np.array_equal(a, b) for a, b in zip(psi.tensors, unit_mps(n, prof, np.random.default_rng(41)).tensors))  # the state is untouched


def test_composition_is_the_operator_product():
    n = 7
    rng = np.random.default_rng(42)
    psi = unit_mps(n, [1, 2, 4, 6, 5, 4, 2, 1], rng)
    A, B = random_dense_mpo(rng, [1, 2, 3, 2, 3, 2, 2, 1]), engine.mpo_from_terms(n, heisenberg_terms(n)).scale(0.1)
    two, one = psi.apply_mpo(A).apply_mpo(B), psi.apply_mpo(B @ A)
    assert list(two.bond_dims()) == list(one.bond_dims())
    assert np.abs(dense(two) - dense(one)).max() <= 1e-12
    assert np.abs(dense(two) - B.to_dense() @ (A.to_dense() @ dense(psi))).max() <= 1e-12


@pytest.mark.parametrize("sign", [+1, -1])
@pytest.mark.parametrize("qubits", [None, (1, 4, 5), (3,), (6, 0)])
def test_parity_projector(sign, qubits):
    n = 7
    rng = np.random.default_rng(43)
    psi = unit_mps(n, [1, 2, 4, 6, 5, 4, 2, 1], rng)
    P = engine.mpo_parity_projector(n, sign, qubits)
    qs = sorted(range(n) if qubits is None else qubits)
    want_bonds = [2 if qs[0] < k <= qs[-1] else 1 for k in range(n + 1)]
    assert list(P.bonds) == want_bonds
    for k in range(n):  # bond 1 outside the hull means the exact identity there
        if k < qs[0] or k > qs[-1]:
            assert np.array_equal(P.tensors[k], np.eye(2).reshape(1, 1, 2, 2))
    z = np.array([1.0])
    for k in range(n):
        z = np.kron(z, np.array([1.0, -1.0]) if k in qs else np.ones(2))
    want = 0.5 * (1 + sign * z) * dense(psi)
    once = psi.apply_mpo(P)
    twice = once.apply_mpo(P)
    assert np.abs(dense(once) - want).max() <= 1e-12
    assert np.abs(dense(twice) - dense(once)).max() <= 1e-12
    assert np.abs(P.to_dense() - np.diag(0.5 * (1 + sign * z))).max() == 0.0
    other = psi.apply_mpo(engine.mpo_parity_projector(n, -sign, qubits))
    assert abs(np.vdot(dense(other), dense(once))) <= 1e-12  # the two sectors are orthogonal
    assert np.abs(dense(other) + dense(once) - dense(psi)).max() <= 1e-12


GATE_CASES = {  # name: (a, b, matrix name or None for Haar, expected bond)
    "adjacent": (3, 4, None, 4),
    "distant": (1, 6, None, 4),
    "reversed": (6, 2, None, 4),
    "reversed adjacent": (5, 4, None, 4),
    "ends": (0, 7, None, 4),
    "CX distant": (2, 5, "CX", 2),
    "CX reversed": (6, 1, "CX", 2),
}


@pytest.mark.parametrize("name", list(GATE_CASES))
def test_two_qubit_gate_against_the_routed_circuit(built, name):
    n = 8
    a, b, which, bond = GATE_CASES[name]
    rng = np.random.default_rng(44)
    U = haar(rng, 4) if which is None else np.array(NAMED[which], dtype=complex)
    gates = brickwork(n, 2, features(1, n, 6)[0], seed=8)  # two Haar layers: bonds <= 4, nothing is truncated
    psi = Q.simulate(from_gates(n, gates), 1.0 - 1e-16)
    want = Q.simulate(from_gates(n, gates + [("Unitary2q", [a, b], [U])]), 1.0 - 1e-16)
    assert psi.fidelity == 1.0 and want.fidelity == 1.0
    G = engine.mpo_two_qubit_gate(n, a, b, U)
    lo, hi = min(a, b), max(a, b)
    assert list(G.bonds) == [bond if lo < k <= hi else 1 for k in range(n + 1)]
    for k in range(n):
        if k < lo or k > hi:
            assert np.array_equal(G.tensors[k], np.eye(2).reshape(1, 1, 2, 2))
        elif lo < k < hi:
            assert np.array_equal(G.tensors[k], np.eye(bond)[:, :, None, None] * np.eye(2)[None, None])
    got = psi.apply_mpo(G)
    x, y = dense(got), dense(want)
    ov = abs(np.vdot(y, x)) / (np.linalg.norm(x) * np.linalg.norm(y))
    print(f"{name}: bond {bond}, normalised overlap modulus = 1 - {1 - ov:.3e}, max |d| = {np.abs(x - y).max():.3e}")
    assert abs(ov - 1) <= 1e-10
    assert np.abs(x - y).max() <= 1e-10  # the phase too: the gate is the same operator, not a ray


def test_index_convention_on_two_sites():
    """Rows are u-major (u chi_k + a), columns v-major (v chi_{k+1} + b); W[u][v][s'][s] maps the ket s to s'."""
    A0 = (np.arange(1, 7) + 1j * np.arange(6)).reshape(1, 2, 3).astype(complex)  # [1][s][b]
    A1 = (np.arange(1, 7)[::-1] - 2j * np.arange(6)).reshape(3, 2, 1).astype(complex)
    W0 = np.zeros((1, 2, 2, 2), dtype=complex)
    W1 = np.zeros((2, 1, 2, 2), dtype=complex)
    W0[0, 0] = [[1, 2], [3, 4]]
    W0[0, 1] = [[0, 1j], [0, 0]]  # only <0| . |1>
    W1[0, 0] = [[1, 0], [0, -1]]
    W1[1, 0] = [[0, 0], [5, 0]]  # only <1| . |0>
    out = Q.MPS([A0, A1]).apply_mpo(engine.Mpo([W0, W1]))
    B0, B1 = out.tensors
    assert B0.shape == (1, 2, 6) and B1.shape == (6, 2, 1)
    for b in range(3):
        # v = 0 block at columns 0..2: s' = 0 row is 1 A[s=0] + 2 A[s=1]; v = 1 block at columns 3..5: s' = 0 is 1j A[s=1], s' = 1 is 0
        assert B0[0, 0, b] == 1 * A0[0, 0, b] + 2 * A0[0, 1, b] and B0[0, 1, b] == 3 * A0[0, 0, b] + 4 * A0[0, 1, b]
        assert B0[0, 0, 3 + b] == 1j * A0[0, 1, b] and B0[0, 1, 3 + b] == 0
    for a in range(3):
        # u = 0 block at rows 0..2, u = 1 block at rows 3..5
        assert B1[a, 0, 0] == A1[a, 0, 0] and B1[a, 1, 0] == -A1[a, 1, 0]
        assert B1[3 + a, 0, 0] == 0 and B1[3 + a, 1, 0] == 5 * A1[a, 0, 0]


def test_errors():
    psi = Q.random_mps(4, [1, 2, 2, 2, 1], np.random.default_rng(0))
    with pytest.raises(ValueError, match="takes an engine.Mpo"):
        psi.apply_mpo([np.eye(2)])
    with pytest.raises(ValueError, match="has 5 sites, the state has 4"):
        psi.apply_mpo(engine.mpo_parity_projector(5))
    for kwargs, match in (
        (dict(n_sites=0), "n_sites >= 1"),
        (dict(n_sites=4, sign=0), "sign must be"),
        (dict(n_sites=4, sign=True), "sign must be"),
        (dict(n_sites=4, sign=2.0), "sign must be"),
        (dict(n_sites=4, qubits=[]), "empty"),
        (dict(n_sites=4, qubits=[1, 1]), "named twice"),
        (dict(n_sites=4, qubits=[4]), "qubit 4 is outside a register of 4"),
        (dict(n_sites=4, qubits=[-1]), "outside"),
        (dict(n_sites=4, qubits="ab"), "sequence of ints"),
    ):
        with pytest.raises(ValueError, match=match):
            engine.mpo_parity_projector(**kwargs)
    U = np.eye(4)
    for args, match in (
        ((4, 1, 1, U), "named twice"),
        ((4, 0, 4, U), "qubit 4 is outside"),
        ((4, -1, 2, U), "outside"),
        ((4, 0, 1, np.eye(2)), "finite 4 x 4"),
        ((4, 0, 1, np.full((4, 4), np.nan)), "finite 4 x 4"),
        ((4, 0, 1, np.zeros((4, 4))), "U is zero"),
        ((4, 0, 1, "x"), "4 x 4"),
    ):
        with pytest.raises(ValueError, match=match):
            engine.mpo_two_qubit_gate(*args)
    # terms at or below 1e-14 sigma_0 are dropped: a product operator plus dust has bond 1
    X, Z = np.array([[0, 1], [1, 0]], dtype=complex), np.diag([1.0, -1.0]).astype(complex)
    assert list(engine.mpo_two_qubit_gate(3, 0, 2, np.kron(X, Z) + 1e-16 * np.kron(Z, X)).bonds) == [1, 1, 1, 1]
    assert list(engine.mpo_two_qubit_gate(3, 0, 2, np.kron(X, Z) + 1e-3 * np.kron(Z, X)).bonds) == [1, 2, 2, 1]


def test_library_exports_the_entry_point(built):
    assert hasattr(engine.lib(), "qk_mps_set_apply_mpo")
    assert engine.Context.apply_mpo.__doc__ and engine.Context.operator_matrix.__doc__
