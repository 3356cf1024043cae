"""Matrix gates on the host (no GPU): op codes 8 (a 2x2 on one qubit) and 9 (a 4x4 on an adjacent pair) through both host builders
against a dense state-vector simulator -- global phase included --, the named constants (X .. SXdg, CX, CY, CZ), the routing of a
non-symmetric gate on reversed and non-adjacent qubits, ``BoundCircuit.from_gates`` / ``as_tuples`` / ``sliced`` / pickling,
``CircuitAnsatz`` templates with constant matrices, gate-list ansatzes with data-dependent matrices, the rejections, and a capped
build.  The dense simulator, the Haar unitaries and the circuits of this file are shared with tests/test_gpu_matrix_gates.py."""
import math
import pickle
from types import SimpleNamespace

import numpy as np
import pytest


_S2 = math.sqrt(0.5)
_W = complex(_S2, _S2)  # e^{i pi / 4}
NAMED = {  # TKET's matrices of the named constants, written out here: the reference of this file, independent of the table under test
    "X": [[0, 1], [1, 0]],
    "Y": [[0, -1j], [1j, 0]],
    "Z": [[1, 0], [0, -1]],
    "S": [[1, 0], [0, 1j]],
    "Sdg": [[1, 0], [0, -1j]],
    "T": [[1, 0], [0, _W]],
    "Tdg": [[1, 0], [0, _W.conjugate()]],
    "V": [[_S2, -1j * _S2], [-1j * _S2, _S2]],
    "Vdg": [[_S2, 1j * _S2], [1j * _S2, _S2]],
    "SX": [[0.5 + 0.5j, 0.5 - 0.5j], [0.5 - 0.5j, 0.5 + 0.5j]],
    "SXdg": [[0.5 - 0.5j, 0.5 + 0.5j], [0.5 + 0.5j, 0.5 - 0.5j]],
    "CX": [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]],  # control first
    "CY": [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, -1j], [0, 0, 1j, 0]],
    "CZ": [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, -1]],
}


# ---- a dense state-vector simulator that knows the matrix gates: psi is an array of shape [2] * n, qubit 0 the first axis
def gate_matrix(name, param):
    """TKET's matrix of a named gate (theta = pi alpha / 2), or the matrix itself for Unitary1q / Unitary2q."""
    if name in ("Unitary1q", "Unitary2q"):
        return np.asarray(param, dtype=complex)
    if name in NAMED:
        return np.array(NAMED[name], dtype=complex)
    if name == "H":
        return np.array([[1, 1], [1, -1]], dtype=complex) / math.sqrt(2.0)
    if name == "SWAP":
        return np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=complex)
    th = math.pi * float(param) / 2.0
    c, s = math.cos(th), math.sin(th)
    if name == "Rz":
        return np.diag([np.exp(-1j * th), np.exp(1j * th)])
    if name == "Rx":
        return np.array([[c, -1j * s], [-1j * s, c]])
    if name == "Ry":
        return np.array([[c, -s], [s, c]], dtype=complex)
    if name == "ZZPhase":
        return np.diag([np.exp(-1j * th), np.exp(1j * th), np.exp(1j * th), np.exp(-1j * th)])
    pauli = {"XXPhase": np.array([[0, 1], [1, 0]], dtype=complex), "YYPhase": np.array([[0, -1j], [1j, 0]])}[name]
    return c * np.eye(4) - 1j * s * np.kron(pauli, pauli)


def apply_dense(psi, m, qubits):
    """``m`` (2x2 or 4x4, index (s_a, s_b) with the first qubit most significant) on the axes ``qubits`` of ``psi``."""
    k = len(qubits)
    t = np.tensordot(np.asarray(m, dtype=complex).reshape((2,) * (2 * k)), psi, axes=(list(range(k, 2 * k)), list(qubits)))
    return np.moveaxis(t, list(range(k)), list(qubits))


def dense_state(n, gates):
    """U|0...0> of an UNROUTED gate list (name, qubits, params), as a vector of 2^n (qubit 0 most significant)."""
    psi = np.zeros((2,) * n, dtype=complex)
    psi[(0,) * n] = 1.0
    for name, qubits, params in gates:
        psi = apply_dense(psi, gate_matrix(name, params[0] if params is not None and len(params) else None), list(qubits))
    return psi.reshape(-1)


def mps_vector(m):
    v = np.ones((1, 1), dtype=complex)
    for t in m.tensors:
        v = np.tensordot(v, t, axes=(v.ndim - 1, 0))
    return v.reshape(-1)


def haar(rng, d):
    q, r = np.linalg.qr(rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))
    ph = np.diag(r) / np.abs(np.diag(r))
    return q * ph[None, :]


def brickwork(n, layers, x, seed, extras=(), matrix=None):
    """``layers`` brickwork layers of Haar ``Unitary2q`` (seeded) -- pairs (0,1),(2,3),.. then (1,2),.., alternating, every third pair
    given reversed -- with a layer of Rz(x_q) / Ry(x_q) data rotations in between, then the gates of ``extras``.  ``matrix(k, u)``,
    when given, replaces the k-th Haar unitary (a data-dependent matrix)."""
    rng = np.random.default_rng(seed)
    gates, k = [], 0
    for layer in range(layers):
        for a in range(layer % 2, n - 1, 2):
            u = haar(rng, 4)
            if matrix is not None:
                u = matrix(k, u)
            gates.append(("Unitary2q", [a + 1, a] if k % 3 == 2 else [a, a + 1], [u]))
            k += 1
        gates += [("Rz" if (q + layer) % 2 else "Ry", [q], [float(x[q])]) for q in range(n)]
    return gates + list(extras)


def from_gates(n, gates):
    """``BoundCircuit.from_gates`` with the named constants (X .. CZ) switched on, as ``as_bound_circuit`` and ``CircuitAnsatz`` do."""
    from qml_cutensornet_amd.ansatz import BoundCircuit

    return BoundCircuit.from_gates(n, gates, named_constants=True)


def features(npts, n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(npts, n))


def both_builders(c):
    from qml_cutensornet_amd import mps

    return mps._simulate(c, 1.0, 1e-16), mps.simulate_native(c, 1.0, 1e-16)


PREP = [("Ry", [0], [0.37]), ("Rz", [0], [0.21]), ("Ry", [1], [-0.58]), ("Rz", [1], [0.44]), ("XXPhase", [0, 1], [0.3])]  # a generic 2-qubit state


def check_against_dense(n, gates, tol=1e-12):
    c = from_gates(n, gates)
    want = dense_state(n, gates)
    assert abs(np.linalg.norm(want) - 1) < 1e-12
    built = both_builders(c)
    for m in built:
        assert np.abs(mps_vector(m) - want).max() <= tol  # global phase included: no gauge freedom reaches the contracted state
    return c, built


def test_both_host_builders_match_the_dense_vector_on_a_haar_brickwork(built):
    n = 8
    x = features(1, n, 3)[0]
    rng = np.random.default_rng(11)
    extras = [("Unitary2q", [6, 1], [haar(rng, 4)]), ("Unitary1q", [3], [haar(rng, 2)]), ("Unitary2q", [2, 5], [haar(rng, 4)]), ("CX", [7, 4], []), ("Unitary1q", [7], [haar(rng, 2)])]
    gates = brickwork(n, 4, x, seed=5, extras=extras)
    assert sum(g[0] == "Unitary2q" and g[1][0] > g[1][1] for g in gates) >= 4 and sum(abs(g[1][0] - g[1][-1]) > 1 for g in gates) == 3
    c, (a, b) = check_against_dense(n, gates)
    assert {1, 3, 5, 8, 9} <= set(c.op.tolist()) and a.max_bond() == 16 and b.max_bond() == 16


def test_named_gates_are_tkets(built):
    from qml_cutensornet_amd import ansatz as A

    assert set(A._NAMED) == set(NAMED)
    for name, m in NAMED.items():  # the table under test against the matrices written out above
        assert np.abs(np.array(A._NAMED[name], dtype=complex) - np.array(m, dtype=complex)).max() < 1e-16, name
    g = lambda name: gate_matrix(name, None)  # noqa: E731
    for lhs, rhs in ((g("S") @ g("S"), g("Z")), (g("T") @ g("T"), g("S")), (g("V") @ g("V"), -1j * g("X")), (g("SX") @ g("SX"), g("X")), (g("Sdg"), g("S").conj().T),
                     (g("Tdg"), g("T").conj().T), (g("Vdg"), g("V").conj().T), (g("SXdg"), g("SX").conj().T), (g("Y"), 1j * g("X") @ g("Z")),
                     (g("V"), gate_matrix("Rx", 0.5)), (g("SX"), np.array([[1 + 1j, 1 - 1j], [1 - 1j, 1 + 1j]]) / 2)):
        assert np.abs(lhs - rhs).max() < 1e-15
    ih = np.kron(np.eye(2), gate_matrix("H", None))
    assert np.abs(g("CX") - ih @ g("CZ") @ ih).max() < 1e-15
    assert np.abs(g("CY") - np.kron(np.diag([1, 0]), np.eye(2)) - np.kron(np.diag([0, 1]), g("Y"))).max() < 1e-15
    # the same identities through both builders, on a generic state
    # (TKET's V is Rx(1/2), so V.V = Rx(1) = -i X: X up to the global phase -i, which the state carries; SX.SX = X exactly)
    for twice, once, phase in (("S", "Z", 1), ("T", "S", 1), ("V", "X", -1j), ("SX", "X", 1)):
        _, (a, _) = check_against_dense(2, PREP + [(twice, [1], []), (twice, [1], [])])
        _, (b, _) = check_against_dense(2, PREP + [(once, [1], [])])
        assert np.abs(mps_vector(a) - phase * mps_vector(b)).max() < 1e-12
    _, (a, _) = check_against_dense(2, PREP + [("S", [0], []), ("Sdg", [0], [])])
    assert np.abs(mps_vector(a) - dense_state(2, PREP)).max() < 1e-12
    _, (a, an) = check_against_dense(2, PREP + [("CX", [0, 1], [])])
    _, (b, bn) = check_against_dense(2, PREP + [("H", [1], []), ("CZ", [0, 1], []), ("H", [1], [])])
    assert np.abs(mps_vector(a) - mps_vector(b)).max() < 1e-12 and np.abs(mps_vector(an) - mps_vector(bn)).max() < 1e-12
    for name in ("X", "Y", "Z", "Sdg", "Tdg", "Vdg", "SXdg", "CY"):
        check_against_dense(3, PREP + [(name, [1] if len(gate_matrix(name, None)) == 2 else [2, 1], [])])
    # one slot per name (per orientation where the gate is not symmetric), at first use
    c = from_gates(4, [("CX", [0, 1], []), ("S", [2], []), ("CX", [2, 3], []), ("CX", [2, 1], []), ("CZ", [3, 2], []), ("CZ", [0, 1], []), ("S", [0], [])])
    assert c.mat.tolist() == [0, 1, 0, 2, 3, 3, 1] and c.mats.shape == (4, 4, 4) and c.alpha.tolist() == [0.0] * 7


def test_ghz_by_a_cx_chain(built):
    n = 8
    gates = [("H", [0], [])] + [("CX", [q, q + 1], []) for q in range(n - 1)]
    ghz = np.zeros(2 ** n, dtype=complex)
    ghz[0] = ghz[-1] = 1 / math.sqrt(2.0)
    assert np.abs(dense_state(n, gates) - ghz).max() < 1e-15
    _, built_ = check_against_dense(n, gates)
    for m in built_:
        assert m.bond_dims().tolist() == [1] + [2] * (n - 1) + [1]


def test_cx_on_reversed_qubits_has_its_control_first(built):
    n = 5
    prep = [("Ry", [q], [0.2 + 0.17 * q]) for q in range(n)] + [("ZZPhase", [2, 3], [0.4])]
    gates = prep + [("CX", [3, 2], [])]
    want = apply_dense(dense_state(n, prep).reshape((2,) * n), gate_matrix("CX", None), [3, 2]).reshape(-1)  # control 3, target 2
    assert np.abs(dense_state(n, gates) - want).max() == 0
    flipped = apply_dense(dense_state(n, prep).reshape((2,) * n), gate_matrix("CX", None), [2, 3]).reshape(-1)
    assert np.abs(want - flipped).max() > 1e-2  # the two orientations differ on this state
    c, _ = check_against_dense(n, gates)
    assert c.op.tolist()[-1] == 9 and c.q0.tolist()[-1] == 2
    check_against_dense(n, prep + [("CY", [4, 1], [])])  # reversed and non-adjacent


def test_crz_needs_no_matrix_gate(built):
    """CRz(alpha) = Rz_target(alpha / 2) . ZZPhase(-alpha / 2), exactly: diag(1, 1, e^{-i theta}, e^{i theta}), theta = pi alpha / 2."""
    for alpha in (0.7, -1.3):
        th = math.pi * alpha / 2.0
        crz = np.diag([1, 1, np.exp(-1j * th), np.exp(1j * th)])
        want = dense_state(2, PREP + [("Unitary2q", [0, 1], [crz])])
        c = from_gates(2, PREP + [("ZZPhase", [0, 1], [-alpha / 2]), ("Rz", [1], [alpha / 2])])
        assert c.mats is None
        for m in both_builders(c):
            assert np.abs(mps_vector(m) - want).max() < 1e-12
        check_against_dense(2, PREP + [("Unitary2q", [0, 1], [crz])])


def test_from_gates_as_tuples_sliced_and_pickle(built):
    from qml_cutensornet_amd.ansatz import BoundCircuit

    n = 6
    rng = np.random.default_rng(2)
    gates = brickwork(n, 2, features(1, n, 8)[0], seed=9, extras=[("Unitary1q", [4], [haar(rng, 2)]), ("Unitary2q", [5, 2], [haar(rng, 4)]), ("SWAP", [0, 1], [])])
    c = from_gates(n, gates)
    assert c.mat.dtype == np.int32 and c.mats.dtype == np.complex128 and c.mats.shape[1:] == (4, 4) and c.mat.shape == c.op.shape
    assert np.array_equal(c.mat >= 0, c.op >= 8) and (c.mat[c.op < 8] == -1).all() and (c.alpha[c.op >= 8] == 0).all()
    assert sorted(c.mat[c.op >= 8].tolist()) == list(range(c.mats.shape[0]))  # every explicit unitary its own slot, in order
    one = c.op == 8
    assert (c.mats[c.mat[one]][:, 2:, :] == 0).all() and (c.mats[c.mat[one]][:, :, 2:] == 0).all()  # a 2x2 sits in [:2, :2]
    tuples = c.as_tuples()
    assert {t[0] for t in tuples} >= {"Unitary1q", "Unitary2q", "Rz", "Ry", "SWAP"}
    assert all(t[2][0].shape == ((2, 2) if t[0] == "Unitary1q" else (4, 4)) and t[1] == ([t[1][0], t[1][0] + 1] if t[0] == "Unitary2q" else t[1]) for t in tuples if t[0].startswith("Unitary"))
    back = from_gates(n, tuples)
    for f in ("op", "q0", "alpha", "mat", "mats"):
        assert np.array_equal(getattr(back, f), getattr(c, f)), f
    # sliced slices mat and keeps the table; the two halves, one after the other, are the whole
    cut = int(np.flatnonzero(c.op == 9)[3])
    head, tail = c.sliced(0, cut), c.sliced(cut, c.n_gates)
    assert head.mats is c.mats and tail.mats is c.mats and np.array_equal(np.concatenate([head.mat, tail.mat]), c.mat)
    whole = BoundCircuit(n, np.concatenate([head.op, tail.op]), np.concatenate([head.q0, tail.q0]), np.concatenate([head.alpha, tail.alpha]), np.concatenate([head.mat, tail.mat]), c.mats)
    want = dense_state(n, gates)
    for m in both_builders(whole):
        assert np.abs(mps_vector(m) - want).max() < 1e-12
    c2 = pickle.loads(pickle.dumps(c))
    for f in ("op", "q0", "alpha", "mat", "mats"):
        assert np.array_equal(getattr(c2, f), getattr(c, f))
    # positional construction as before the matrix gates: no table
    plain = BoundCircuit(2, np.array([0, 2], dtype=np.int8), np.array([0, 0], dtype=np.int32), np.array([0.0, 0.3]))
    assert plain.mat is None and plain.mats is None and plain.sliced(0, 1).mats is None


def test_checkpointed_numpy_builder_takes_the_matrix_gates(built):
    from qml_cutensornet_amd import mps

    n = 6
    gates = brickwork(n, 3, features(1, n, 4)[0], seed=21, extras=[("CX", [4, 1], [])])
    c = from_gates(n, gates)
    cps = [5, 14, c.n_gates]
    snaps = mps.simulate(c, 1.0, checkpoints=cps)
    assert len(snaps) == 3
    for m, cp in zip(snaps, cps):
        fresh = mps._simulate(c.sliced(0, cp), 1.0, 1e-16)
        assert np.abs(mps_vector(m) - mps_vector(fresh)).max() < 1e-12
    assert np.abs(mps_vector(snaps[-1]) - dense_state(n, gates)).max() < 1e-12


def template(n, rng):
    """A CircuitAnsatz template with constant matrix gates between data-dependent rotations."""
    t = [("H", [q], None) for q in range(n)]
    t += [("Rz", [q], (0.8, (q, 0.0, 1.0))) for q in range(n)]
    t += [("CX", [q, q + 1], None) for q in range(0, n - 1, 2)] + [("CZ", [n - 1, 0], None), ("T", [1], None), ("SXdg", 2, None)]
    t += [("Unitary2q", [3, 1], haar(rng, 4)), ("Unitary1q", [0], haar(rng, 2))]
    t += [("Ry", [q], (0.5, (q, 0.25, 1.0))) for q in range(n)] + [("CX", [2, 1], None), ("ZZPhase", [0, 2], (0.7, (0, 1.0, -1.0), (2, 1.0, -1.0)))]
    return t


def bind_template(t, x):
    out = []
    for name, qs, ang in t:
        qs = [qs] if np.ndim(qs) == 0 else list(qs)
        if ang is None:
            out.append((name, qs, []))
        elif isinstance(ang, np.ndarray):
            out.append((name, qs, [ang]))
        else:
            v = ang[0]
            for a, c, d in ang[1:]:
                v = v * (c + d * x[a])
            out.append((name, qs, [float(v)]))
    return out


def test_circuit_ansatz_binds_constant_matrices(built):
    import qml_cutensornet_amd as Q

    n = 5
    t = template(n, np.random.default_rng(6))
    ca = pickle.loads(pickle.dumps(Q.CircuitAnsatz(n, t)))
    X = features(3, n, 12)
    bound = [ca.circuit_for_data(x) for x in X]
    assert all(b.mats is bound[0].mats and b.mat is bound[0].mat for b in bound)  # one table, shared by every data point
    for b, x in zip(bound, X):
        via_list = from_gates(n, bind_template(t, x))
        for f in ("op", "q0", "mat", "mats"):
            assert np.array_equal(getattr(b, f), getattr(via_list, f)), f
        assert np.abs(b.alpha - via_list.alpha).max() < 1e-14
        want = dense_state(n, bind_template(t, x))
        for m in both_builders(b):
            assert np.abs(mps_vector(m) - want).max() < 1e-12
    with pytest.raises(ValueError):
        Q.CircuitAnsatz(3, [("CX", [0, 1], 0.5)])  # a named constant takes no angle
    with pytest.raises(ValueError):
        Q.CircuitAnsatz(3, [("Unitary1q", [0], None)])
    with pytest.raises(ValueError):
        Q.CircuitAnsatz(3, [("Unitary2q", [0, 1], np.eye(2))])
    plain = Q.CircuitAnsatz(3, [("H", [0], None), ("ZZPhase", [0, 1], 0.3)]).circuit_for_data(np.zeros(3))
    assert plain.mat is None and plain.mats is None


class MatrixGateList:
    """A gate-list ansatz (``circuit_for_data`` returns (name, qubits, params)) whose matrices depend on the data point:
    a ``Unitary1q`` Rz(x_q)-like phase gate per qubit and the brickwork with every Haar unitary multiplied by a data-dependent
    diagonal."""

    def __init__(self, n, layers, seed, extras=()):
        self.n, self.layers, self.seed, self.extras = n, layers, seed, list(extras)
        self.ansatz_circ = SimpleNamespace(n_qubits=n)
        self.feature_symbol_list = [f"f_{i}" for i in range(n)]

    def circuit_for_data(self, x):
        if len(x) != self.n:
            raise RuntimeError("The number of values must match the number of symbols.")
        x = np.asarray(x, dtype=float)
        dep = lambda k, u: u @ np.diag(np.exp(1j * x[k % self.n] * np.arange(4)))  # noqa: E731
        gates = [("H", [q], []) for q in range(self.n)]
        gates += [("Unitary1q", [q], [np.array([[np.cos(x[q]), -np.sin(x[q])], [np.sin(x[q]), np.cos(x[q])]]) @ np.diag([1, np.exp(1j * x[q])])]) for q in range(self.n)]
        return gates + brickwork(self.n, self.layers, x, self.seed, self.extras, matrix=dep)


def test_gate_list_ansatz_with_data_dependent_matrices(built):
    from qml_cutensornet_amd.ansatz import as_bound_circuit
    from qml_cutensornet_amd.builder_pool import build_states
    from qml_cutensornet_amd.gpu_backend import kernel_state_ansatz as G

    n = 6
    gl = MatrixGateList(n, 2, seed=4, extras=[("CX", [5, 2], [])])
    X = features(3, n, 30)
    a, b = (as_bound_circuit(gl.circuit_for_data(x), gl) for x in X[:2])
    for f in ("op", "q0", "mat"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert a.mats.shape == b.mats.shape and not np.array_equal(a.mats, b.mats)
    want = [dense_state(n, gl.circuit_for_data(x)) for x in X]
    lo, states, _, fid = G._simulate_share(gl, X, 0, 1, 1 - 1e-16, False, "X", want_set=False)  # the share builder hands the table on
    pooled, _ = build_states(gl, X, 1 - 1e-16, workers=2)  # ... and so do the pool's workers
    assert lo == 0 and all(abs(f - 1) < 1e-12 for f in fid)
    for group in (states, pooled):
        for m, w in zip(group, want):
            assert np.abs(mps_vector(m) - w).max() < 1e-12


def test_pool_worker_processes_take_the_table(built, monkeypatch):
    from qml_cutensornet_amd import mps

    n = 5
    X = features(3, n, 2)
    lists = [brickwork(n, 2, x, seed=8, extras=[("CX", [3, 0], [])]) for x in X]
    monkeypatch.setenv("QK_BUILDER_POOL", "procs")
    built_, _ = mps.simulate_many([from_gates(n, g) for g in lists], workers=2)
    for m, g in zip(built_, lists):
        assert np.abs(mps_vector(m) - dense_state(n, g)).max() < 1e-12


def bad_programs():
    """(label, BoundCircuit) pairs every builder must refuse, and the text the message carries."""
    from qml_cutensornet_amd.ansatz import BoundCircuit

    n = 4
    op = np.array([0, 8, 9, 2], dtype=np.int8)
    q0 = np.array([0, 1, 1, 0], dtype=np.int32)
    alpha = np.array([0, 0, 0, 0.3])
    mat = np.array([-1, 0, 1, -1], dtype=np.int32)
    good = np.zeros((2, 4, 4), dtype=np.complex128)
    good[0, :2, :2] = np.array([[0, 1], [1, 0]])
    good[1] = np.eye(4)[[0, 1, 3, 2]]
    out = [("ok", BoundCircuit(n, op, q0, alpha, mat, good), None)]
    shear = good.copy()
    shear[0, :2, :2] = [[1, 1], [0, 1]]
    out.append(("not unitary", BoundCircuit(n, op, q0, alpha, mat, shear), "gate 1"))
    scaled = good.copy()
    scaled[1] *= 1 + 1e-9
    out.append(("not unitary by 2e-9", BoundCircuit(n, op, q0, alpha, mat, scaled), "gate 2"))
    nan = good.copy()
    nan[1, 2, 1] = np.nan
    out.append(("NaN", BoundCircuit(n, op, q0, alpha, mat, nan), "gate 2"))
    out.append(("index out of range", BoundCircuit(n, op, q0, alpha, np.array([-1, 0, 2, -1], dtype=np.int32), good), "gate 2"))
    out.append(("negative index", BoundCircuit(n, op, q0, alpha, np.array([-1, -1, 1, -1], dtype=np.int32), good), "gate 1"))
    out.append(("M2 on the last qubit", BoundCircuit(n, op, np.array([0, 1, 3, 0], dtype=np.int32), alpha, mat, good), "outside"))
    out.append(("no table", BoundCircuit(n, op, q0, alpha), "op code"))
    out.append(("code 10", BoundCircuit(n, np.array([0, 8, 10, 2], dtype=np.int8), q0, alpha, mat, good), "op code"))
    small = np.zeros((2, 2, 2), dtype=np.complex128)  # a table of bare 2x2 slots: the wrong shape
    small[:] = np.eye(2)
    out.append(("table of the wrong shape", BoundCircuit(n, op, q0, alpha, mat, small), "matrix table must be"))
    out.append(("flat table", BoundCircuit(n, op, q0, alpha, mat, good.reshape(2, 16)), "matrix table must be"))
    out.append(("mat of the wrong length", BoundCircuit(n, op, q0, alpha, mat[:3], good), "one index per gate"))
    return out


N_BAD = 11  # the cases of bad_programs() behind its first, good one


@pytest.mark.parametrize("case", range(1, N_BAD + 1))
def test_host_builders_reject_bad_matrix_gates(built, case):
    from qml_cutensornet_amd import mps

    assert len(bad_programs()) == N_BAD + 1
    label, ok, _ = bad_programs()[0]
    assert all(abs(m.fidelity - 1) < 1e-12 for m in both_builders(ok))  # the same program with a good table runs
    label, c, text = bad_programs()[case]
    with pytest.raises(ValueError, match=text):
        mps._simulate(c, 1.0, 1e-16)
    with pytest.raises((ValueError, RuntimeError) if "last qubit" in label else ValueError, match=text):
        mps.simulate_native(c, 1.0)
    if "last qubit" not in label:
        with pytest.raises(ValueError, match=text):
            c.as_tuples()


def test_from_gates_rejects_bad_matrix_gates():
    from qml_cutensornet_amd.ansatz import BoundCircuit

    for gates in ([("Unitary1q", [0], [np.array([[1, 1], [0, 1]])])],        # not unitary
                  [("Unitary1q", [0], [np.array([[1, 0], [0, np.nan]])])],     # NaN
                  [("Unitary2q", [0, 1], [np.eye(2)])],                        # wrong shape
                  [("Unitary1q", [0], [np.eye(4)])],
                  [("Unitary2q", [0, 1], [np.eye(4), np.eye(4)])],
                  [("Unitary2q", [0, 1], [])],
                  [("Unitary1q", [0, 1], [np.eye(2)])],                        # Unitary1q on two qubits
                  [("Unitary2q", [1], [np.eye(4)])],
                  [("Unitary2q", [2, 2], [np.eye(4)])],
                  [("CX", [0, 4], [])],                                        # outside the register
                  [("CX", [0, 1], [0.5])],                                     # a named constant takes no parameter
                  [("S", [0, 1], [])],
                  [("CCX", [0, 1], [])]):
        with pytest.raises(ValueError):
            from_gates(4, gates)
    with pytest.raises(ValueError, match="gate 1"):
        from_gates(4, [("H", [0], []), ("Unitary2q", [0, 1], [2 * np.eye(4)])])
    assert from_gates(4, [("Unitary2q", [0, 1], np.eye(4))]).mats.shape == (1, 4, 4)  # the bare matrix is accepted too
    # the named constants are opt-in in a direct call (the plain vocabulary stays the op-code names); explicit unitaries are not
    with pytest.raises(ValueError, match="named_constants"):
        BoundCircuit.from_gates(4, [("CX", [0, 1], [])])
    assert BoundCircuit.from_gates(4, [("Unitary2q", [1, 0], [np.eye(4)])]).op.tolist() == [9]


def test_capped_build_in_both_host_builders(built):
    """The Haar brickwork cut at bond 4: both builders truncate (fidelity < 1) to the same bonds, the same fidelity product and the same
    state -- the tolerances of tests/test_host_logic.py::test_native_builder_matches_numpy_builder for these two builders."""
    from oracle import restatement as R
    from qml_cutensornet_amd import mps

    n = 8
    gates = brickwork(n, 4, features(1, n, 3)[0], seed=5, extras=[("CX", [6, 3], [])])
    c = from_gates(n, gates)
    a = mps._simulate(c, 1 - 1e-16, 1e-16, max_bond=4)
    b = mps.simulate_native(c, 1 - 1e-16, 1e-16, max_bond=4)
    assert a.max_bond() == 4 and b.max_bond() == 4 and a.fidelity < 1 - 1e-3 and b.fidelity < 1 - 1e-3
    assert (a.bond_dims() == b.bond_dims()).all()
    assert abs(a.fidelity - b.fidelity) < 1e-12
    assert abs(abs(R.mps_inner(a.tensors, b.tensors)) - 1) < 1e-12
    free = mps._simulate(c, 1 - 1e-16, 1e-16)
    assert free.max_bond() == 16 and abs(R.mps_inner(a.tensors, free.tensors)) ** 2 < 1 - 1e-3  # the cap changed the state


def test_cost_proxy_counts_the_4x4_matrix_gates(built):
    """The builder policies' cost proxy: sin^2(pi alpha) per XX / YY / ZZ gate as before, plus 1 per 4x4 matrix gate (a SWAP of the
    routing and a 2x2 add nothing), so a circuit of matrix gates no longer weighs 0 and is not expected to keep small bonds."""
    from qml_cutensornet_amd.gpu_backend import kernel_state_ansatz as G

    c = from_gates(6, [("ZZPhase", [0, 1], [0.5]), ("CX", [0, 1], []), ("Unitary2q", [4, 1], [np.eye(4)]), ("S", [2], []), ("Unitary1q", [3], [np.eye(2)])])
    assert c.op.tolist().count(9) == 2 and c.op.tolist().count(3) == 4
    assert abs(G._entangling_weight(c) - 3.0) < 1e-12
    deep = from_gates(12, brickwork(12, 6, features(1, 12, 1)[0], seed=3))
    assert G._entangling_weight(deep) == 33.0 and not G._expect_small_bonds(SimpleNamespace(), [deep])
    assert G._auto_builder([deep] * 40, 1) == "device" and G._auto_builder([deep] * 3, 2) == "host"

