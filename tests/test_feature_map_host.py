"""Custom feature maps on the host: the gate vocabulary H, Rz, Rx, Ry, XXPhase, YYPhase, ZZPhase, SWAP (op codes 0-7)
through both host builders against exact state vectors, ``CircuitAnsatz`` against ``KernelStateAnsatz``,
``BoundCircuit.from_gates`` / ``as_tuples``, the rejection of unknown op codes, and the builder pools (no GPU)."""
import math
import pickle
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import restatement as R

NAMES_1Q = ("H", "Rz", "Rx", "Ry")
NAMES_2Q = ("XXPhase", "YYPhase", "ZZPhase", "SWAP")


def _gate_matrix_ext(orig):
    """The oracle's TKET matrices plus the two it does not state: Ry and YYPhase (theta = pi alpha / 2)."""

    def gm(name, alpha):
        if name in ("Ry", "YYPhase"):
            th = math.pi * alpha / 2.0
            c, s = math.cos(th), math.sin(th)
            if name == "Ry":
                return np.array([[c, -s], [s, c]], dtype=complex)
            return np.array([[c, 0, 0, 1j * s], [0, c, -1j * s, 0], [0, -1j * s, c, 0], [1j * s, 0, 0, c]])
        return orig(name, alpha)

    return gm


@pytest.fixture
def exact(monkeypatch):
    """Dense U|0...0> of an UNROUTED reference-style gate list (any qubit pair, either order)."""
    monkeypatch.setattr(R, "gate_matrix", _gate_matrix_ext(R.gate_matrix))

    def sv(n, gates):
        return R.statevector(n, [(name, tuple(qs), (p[0] if p else None)) for name, qs, p in gates])

    return sv


def dense(mps):
    v = np.ones((1, 1), dtype=complex)
    for t in mps.tensors:
        v = np.tensordot(v, t, axes=(v.ndim - 1, 0))
    return v.reshape(-1)


def random_gates(rng, n, n_gates, hadamard_layer):
    gates = [("H", [q], []) for q in range(n)] if hadamard_layer else []
    for _ in range(n_gates):
        if rng.random() < 0.45:
            name = NAMES_1Q[rng.integers(4)]
            gates.append((name, [int(rng.integers(n))], [] if name == "H" else [float(rng.uniform(-2, 2))]))
        else:
            name = NAMES_2Q[rng.integers(4)]
            a, b = (int(v) for v in rng.choice(n, 2, replace=False))  # any distance, either order
            gates.append((name, [a, b], [] if name == "SWAP" else [float(rng.uniform(-2, 2))]))
    return gates


@pytest.mark.parametrize("seed", range(6))
def test_both_host_builders_match_exact_statevector(exact, seed):
    from qml_cutensornet_amd import mps
    from qml_cutensornet_amd.ansatz import BoundCircuit

    rng = np.random.default_rng(100 + seed)
    n = 6 + seed % 5
    gates = random_gates(rng, n, 14 + 4 * n, hadamard_layer=seed % 2 == 0)
    for name in NAMES_1Q + NAMES_2Q:  # every op occurs
        assert any(g[0] == name for g in gates) or name == "H"
    c = BoundCircuit.from_gates(n, gates)
    assert set(c.op.tolist()) >= {1, 2, 3, 4, 5, 6, 7}
    want = exact(n, gates)
    assert abs(np.linalg.norm(want) - 1) < 1e-12
    got_np = dense(mps._simulate(c, 1.0, 1e-16))
    got_nat = dense(mps.simulate_native(c, 1.0))
    assert np.abs(got_np - want).max() < 1e-12  # global phase included
    assert np.abs(got_nat - want).max() < 1e-12


@pytest.mark.parametrize("name", ["Rx", "Ry", "Rz", "H"])
def test_single_qubit_gate_on_the_last_qubit(exact, name):
    """A one-qubit gate on qubit n-1 is in range, and it does not move the orthogonality centre."""
    from qml_cutensornet_amd import mps
    from qml_cutensornet_amd.ansatz import BoundCircuit

    n = 5
    gates = [("H", [q], []) for q in range(n)] + [("ZZPhase", [0, 1], [0.7]), ("YYPhase", [3, 2], [0.3]),
                                                  (name, [n - 1], [] if name == "H" else [0.9]), ("XXPhase", [1, 2], [0.4]),
                                                  (name, [0], [] if name == "H" else [-0.6]), ("ZZPhase", [4, 3], [1.3])]
    c = BoundCircuit.from_gates(n, gates)
    want = exact(n, gates)
    for built in (mps._simulate(c, 1.0, 1e-16), mps.simulate_native(c, 1.0)):
        assert np.abs(dense(built) - want).max() < 1e-12


def reference_template(n, reps, gamma, edges):
    gates = [("H", [q], None) for q in range(n)]
    for _ in range(reps):
        gates += [("Rz", [q], ((2.0 / np.pi) * gamma, (q, 0.0, 1.0))) for q in range(n)]
        gates += [("XXPhase", [a, b], (gamma * gamma, (a, 1.0, -1.0), (b, 1.0, -1.0))) for a, b in edges]
    return gates


def test_circuit_ansatz_reproduces_the_reference_ansatz_exactly():
    import qml_cutensornet_amd as Q

    n, reps, gamma, d = 11, 3, 0.8, 4
    e = Q.entanglement_graph(n, d)
    ref = Q.KernelStateAnsatz(n, reps, gamma, e)
    ca = Q.CircuitAnsatz(n, reference_template(n, reps, gamma, e))
    assert ca.ansatz_circ.n_qubits == n and ca.feature_symbol_list == ref.feature_symbol_list
    for x in R.synthetic_features(4, n, 3):
        a, b = ca.circuit_for_data(x), ref.circuit_for_data(x)
        assert np.array_equal(a.op, b.op) and np.array_equal(a.q0, b.q0)
        assert np.array_equal(a.alpha, b.alpha)
    with pytest.raises(RuntimeError):
        ca.circuit_for_data(np.zeros(n - 1))


def test_from_gates_matches_the_ansatz_program_and_round_trips():
    import qml_cutensornet_amd as Q
    from qml_cutensornet_amd.ansatz import BoundCircuit

    n, reps, gamma, d = 11, 3, 0.8, 4
    e = Q.entanglement_graph(n, d)
    ref = Q.KernelStateAnsatz(n, reps, gamma, e)
    x = R.synthetic_features(3, n, 3)[1]
    gates = [("H", [q], []) for q in range(n)]
    for _ in range(reps):  # the UNROUTED gate list of the reference's CPU backend
        gates += [("Rz", [q], [(2.0 / np.pi) * gamma * x[q]]) for q in range(n)]
        gates += [("XXPhase", [a, b], [gamma * gamma * (1.0 - x[a]) * (1.0 - x[b])]) for a, b in e]
    c, want = BoundCircuit.from_gates(n, gates), ref.circuit_for_data(x)
    assert np.array_equal(c.op, want.op) and np.array_equal(c.q0, want.q0) and np.array_equal(c.alpha, want.alpha)
    rng = np.random.default_rng(5)
    for circ in (want, BoundCircuit.from_gates(9, random_gates(rng, 9, 60, True))):
        back = BoundCircuit.from_gates(circ.n_qubits, circ.as_tuples())
        assert np.array_equal(back.op, circ.op) and np.array_equal(back.q0, circ.q0) and np.array_equal(back.alpha, circ.alpha)
    names = {g[0] for g in BoundCircuit.from_gates(9, random_gates(rng, 9, 80, True)).as_tuples()}
    assert names == set(NAMES_1Q + NAMES_2Q)
    with pytest.raises(ValueError):
        BoundCircuit.from_gates(4, [("CX", [0, 1], [])])
    with pytest.raises(ValueError):
        BoundCircuit.from_gates(4, [("ZZPhase", [0, 4], [0.1])])
    with pytest.raises(ValueError):
        BoundCircuit.from_gates(4, [("Rx", [0, 1], [0.1])])


@pytest.mark.parametrize("code", [8, -1])
def test_host_builders_reject_unknown_op_codes(code):
    """An op code outside 0..7 is an error in both host builders (it used to be applied as an XXPhase)."""
    from qml_cutensornet_amd import mps
    from qml_cutensornet_amd.ansatz import BoundCircuit

    n = 4
    op = np.array([0, 0, 0, 0, code, 2], dtype=np.int8)
    q0 = np.array([0, 1, 2, 3, 1, 0], dtype=np.int32)
    c = BoundCircuit(n, op, q0, np.array([0, 0, 0, 0, 0.6, 0.3]))
    with pytest.raises(ValueError, match="op code"):
        mps._simulate(c, 1.0, 1e-16)
    with pytest.raises(ValueError, match="op code"):
        mps.simulate_native(c, 1.0)
    with pytest.raises(ValueError):
        c.as_tuples()


def zz_template(n, layers, gamma, nn):
    """A Havlicek-style ZZ map with Rx / Ry encodings and YYPhase couplers (pairs up to distance nn, some reversed)."""
    g = []
    for layer in range(layers):
        g += [("H", [q], None) for q in range(n)]
        g += [("Rz", [q], (gamma, (q, 0.0, 1.0))) for q in range(n)]
        g += [("Ry" if q % 2 else "Rx", [q], (0.5 * gamma, (q, 0.25, 1.0))) for q in range(n)]
        for dist in range(1, nn + 1):
            for a in range(n - dist):
                b = a + dist
                pair = [b, a] if (a + layer) % 3 == 0 else [a, b]
                g.append(("ZZPhase", pair, (gamma, (a, np.pi, -1.0), (b, np.pi, -1.0))))
                if dist == 1:
                    g.append(("YYPhase", pair, (0.3 * gamma, (a, 1.0, -1.0))))
        g.append(("Rx", [n - 1], 0.25))  # a constant angle
    return g


class GateListAnsatz:
    """An ansatz in the reference CPU backend's shape: ``circuit_for_data`` returns (name, qubits, params) lists."""

    def __init__(self, n, template):
        self.template = template
        self.ansatz_circ = SimpleNamespace(n_qubits=n)
        self.feature_symbol_list = [f"f_{i}" for i in range(n)]

    def circuit_for_data(self, x):
        if len(x) != len(self.feature_symbol_list):
            raise RuntimeError("The number of values must match the number of symbols.")
        out = []
        for name, qs, ang in self.template:
            if ang is None:
                out.append((name, list(qs), []))
            elif not isinstance(ang, tuple):
                out.append((name, list(qs), [float(ang)]))
            else:
                v = ang[0]
                for a, c, d in ang[1:]:
                    v = v * (c + d * x[a])
                out.append((name, list(qs), [float(v)]))
        return out


def test_circuit_ansatz_against_exact_statevector_and_gate_lists(exact):
    import qml_cutensornet_amd as Q
    from qml_cutensornet_amd.ansatz import BoundCircuit

    n = 7
    tmpl = zz_template(n, 2, 0.7, 2)
    ca, gl = Q.CircuitAnsatz(n, tmpl), GateListAnsatz(n, tmpl)
    for x in R.synthetic_features(3, n, 9):
        c = ca.circuit_for_data(x)
        via_list = BoundCircuit.from_gates(n, gl.circuit_for_data(x))
        assert np.array_equal(c.op, via_list.op) and np.array_equal(c.q0, via_list.q0)
        assert np.abs(c.alpha - via_list.alpha).max() < 1e-14
        want = exact(n, gl.circuit_for_data(x))
        assert np.abs(dense(Q.simulate(c, 1.0)) - want).max() < 1e-12


def test_circuit_ansatz_bad_templates():
    import qml_cutensornet_amd as Q

    with pytest.raises(ValueError):
        Q.CircuitAnsatz(3, [("Rz", [0], (1.0, (3, 0.0, 1.0)))])  # feature 3 of 3
    with pytest.raises(ValueError):
        Q.CircuitAnsatz(3, [("H", [0], 0.5)])
    with pytest.raises(ValueError):
        Q.CircuitAnsatz(3, [("Rz", [0], None)])
    with pytest.raises(ValueError):
        Q.CircuitAnsatz(3, [("CZ", [0, 1], 0.5)])
    ca = Q.CircuitAnsatz(2, [("Rx", [0], (1.0, (3, 0.0, 1.0)))], num_features=4)
    assert ca.feature_symbol_list == ["f_0", "f_1", "f_2", "f_3"]
    assert ca.circuit_for_data([0, 0, 0, 0.5]).alpha.tolist() == [0.5]


def test_circuit_ansatz_pickles_and_the_pools_agree(monkeypatch):
    import qml_cutensornet_amd as Q
    from qml_cutensornet_amd import mps
    from qml_cutensornet_amd.builder_pool import build_states

    n = 8
    ca = Q.CircuitAnsatz(n, zz_template(n, 2, 0.6, 2))
    ca2 = pickle.loads(pickle.dumps(ca))
    X = R.synthetic_features(6, n, 21)
    circuits = [ca.circuit_for_data(x) for x in X]
    for c, x in zip(circuits, X):
        c2 = ca2.circuit_for_data(x)
        assert np.array_equal(c.op, c2.op) and np.array_equal(c.q0, c2.q0) and np.array_equal(c.alpha, c2.alpha)
    monkeypatch.setenv("QK_BUILDER_POOL", "serial")
    serial, _ = mps.simulate_many(circuits, workers=3)
    monkeypatch.setenv("QK_BUILDER_POOL", "procs")
    procs, _ = mps.simulate_many(circuits, workers=3)
    forked, _ = build_states(GateListAnsatz(n, zz_template(n, 2, 0.6, 2)), X, 1 - 1e-16, workers=2)
    for a, b, f in zip(serial, procs, forked):
        assert a.max_bond() > 2
        for ta, tb, tf in zip(a.tensors, b.tensors, f.tensors):
            assert ta.shape == tb.shape == tf.shape
            assert np.abs(ta - tb).max() < 1e-13 and np.abs(ta - tf).max() < 1e-13


def test_share_builder_and_cost_proxy_take_gate_lists():
    """build_kernel_matrix's share builder (host path) accepts an ansatz that returns gate lists; the cost proxy counts
    XX, YY and ZZ and is unchanged for the reference ansatz."""
    import qml_cutensornet_amd as Q
    from qml_cutensornet_amd.gpu_backend import kernel_state_ansatz as G

    n = 6
    tmpl = zz_template(n, 1, 0.5, 1)
    X = R.synthetic_features(3, n, 4)
    lo, states, _, fid = G._simulate_share(GateListAnsatz(n, tmpl), X, 0, 1, 1 - 1e-16, False, "X", want_set=False)
    ca = Q.CircuitAnsatz(n, tmpl)
    assert lo == 0 and len(states) == 3 and all(abs(f - 1) < 1e-12 for f in fid)
    for m, x in zip(states, X):
        assert np.abs(dense(m) - dense(Q.simulate(ca.circuit_for_data(x)))).max() < 1e-12
    c = Q.BoundCircuit.from_gates(3, [("XXPhase", [0, 1], [0.5]), ("YYPhase", [1, 2], [0.5]), ("ZZPhase", [0, 2], [0.5]), ("Rx", [0], [0.5])])
    assert abs(G._entangling_weight(c) - 3.0) < 1e-12
    ref = Q.KernelStateAnsatz(n, 2, 1.0, Q.entanglement_graph(n, 2)).circuit_for_data(X[0])
    xx = ref.op == 2
    assert G._entangling_weight(ref) == float((np.sin(np.pi * ref.alpha[xx]) ** 2).sum())
