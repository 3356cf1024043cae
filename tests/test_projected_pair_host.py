"""Two-qubit projected quantum kernel on the host (no GPU): the numpy reference of the pair sweep (reduced density matrices of
neighbouring qubits from left and right environments, as Pauli correlators T[k][p][q]) against dense-state-vector partial
traces, its margins against the one-qubit reference, an analytic XXPhase case, the Frobenius identity behind the Gram, the
argument checks of ``build_projected_kernel_matrix(rdm=...)`` (raised before any device work) and the library's exports."""
import math

import numpy as np
import pytest

import qml_cutensornet_amd as Q
from oracle import restatement as R
from test_projected_host import dense, ref_local_paulis, zz_template

PAULIS = np.array([[[1, 0], [0, 1]], [[0, 1], [1, 0]], [[0, -1j], [1j, 0]], [[1, 0], [0, -1]]], dtype=complex)


# ---- numpy reference (the contract of qk_local_pair_paulis_host) ------------------------------------------------------
def correlators_from_rho(rho):
    """T[p][q] = sum rho[(s,t)][(s',t')] P_p[s'][s] P_q[t'][t] of a two-qubit density matrix given as rho[s][t][s'][t']."""
    T = np.einsum("stuv,pus,qvt->pq", rho, PAULIS, PAULIS)
    assert np.abs(T.imag).max() < 1e-12
    return T.real


def ref_pair_paulis(tensors):
    """Pauli correlators T[k][p][q] = <P_p on k, P_q on k+1>, k = 0 .. n-2, and <psi|psi> of an MPS given as
    [chi_k][2][chi_k+1] complex tensors, from left and right environments."""
    n = len(tensors)
    Rs = [None] * (n + 1)
    Rs[n] = np.ones((1, 1), dtype=complex)
    for k in range(n - 1, -1, -1):
        A = tensors[k]
        Rs[k] = np.einsum("lsr,rq,msq->lm", A, Rs[k + 1], A.conj(), optimize=True)
    norm = Rs[0][0, 0].real
    L = np.ones((1, 1), dtype=complex)
    T = np.zeros((n - 1, 4, 4))
    for k in range(n - 1):
        A, B = tensors[k], tensors[k + 1]
        W = np.einsum("lm,lsr,muq->sruq", L, A, A.conj(), optimize=True)  # W[s][b'][s'][a']
        V = np.einsum("rtc,qvd,cd->trvq", B, B.conj(), Rs[k + 2], optimize=True)  # V[t][b'][t'][a']
        rho = np.einsum("sruq,trvq->stuv", W, V, optimize=True) / norm
        T[k] = correlators_from_rho(rho)
        T[k, 0, 0] = 1.0
        L = np.einsum("lm,lsr,msq->rq", L, A, A.conj(), optimize=True)
    return T, norm


def pair_from_dense(psi, n):
    """T[k][p][q] of every neighbouring pair of a dense state (qubit 0 = most significant axis) by partial traces."""
    psi = np.asarray(psi).reshape((2,) * n)
    norm = float(np.vdot(psi, psi).real)
    T = np.zeros((n - 1, 4, 4))
    for k in range(n - 1):
        m = np.moveaxis(psi, (k, k + 1), (0, 1)).reshape(4, -1)
        rho = (m @ m.conj().T / norm).reshape(2, 2, 2, 2)
        T[k] = correlators_from_rho(rho)
    return T, norm


def ref_pair_gram(tx, ty, g):
    """K_2[j, i] = exp(-g/4 sum_k sum_pq (tx[i, k, p, q] - ty[j, k, p, q])^2)."""
    d = tx[None, :, :, :, :] - ty[:, None, :, :, :]
    return np.exp(-0.25 * g * (d * d).sum(axis=(2, 3, 4)))


def _check_state(m, n):
    T, norm = ref_pair_paulis(m.tensors)
    Td, nd = pair_from_dense(dense(m), n)
    err = np.abs(T - Td).max()
    assert err < 1e-13, err
    assert abs(norm - nd) < 1e-13 * nd
    assert np.all(T[:, 0, 0] == 1.0)
    return T


# ---- the reference against partial traces -------------------------------------------------------------------------
@pytest.mark.parametrize("n,reps,d", [(8, 2, 1), (10, 2, 2), (12, 1, 3)])
def test_pair_reference_matches_partial_trace_kernel_state_ansatz(n, reps, d):
    ans = Q.KernelStateAnsatz(n, reps, 1.0, Q.entanglement_graph(n, d))
    for x in R.synthetic_features(3, n, 11 + n):
        _check_state(Q.simulate(ans.circuit_for_data(x), 1 - 1e-16), n)


@pytest.mark.parametrize("n", [8, 11])
def test_pair_reference_matches_partial_trace_circuit_ansatz(n):
    ca = Q.CircuitAnsatz(n, zz_template(n))
    for x in R.synthetic_features(3, n, 5):
        _check_state(Q.simulate(ca.circuit_for_data(x), 1 - 1e-16), n)


def test_pair_reference_ragged_random_and_unnormalised():
    rng = np.random.default_rng(7)
    for prof in ([1, 2, 4, 8, 13, 9, 5, 3, 2, 1], [1, 2, 3, 6, 11, 7, 4, 2, 1], [1, 2, 1], [1, 1, 1], [1, 2, 2, 1]):
        n = len(prof) - 1
        m = Q.random_mps(n, prof, rng)
        T = _check_state(m, n)
        scaled = [t * (3.7 if k == min(1, n - 1) else 1.0) for k, t in enumerate(m.tensors)]
        Ts, ns = ref_pair_paulis(scaled)
        assert np.abs(Ts - T).max() < 1e-13
        assert abs(ns - 3.7**2 * ref_pair_paulis(m.tensors)[1]) < 1e-12 * ns


def test_pair_margins_are_the_bloch_vectors():
    rng = np.random.default_rng(3)
    ans = Q.KernelStateAnsatz(9, 2, 1.0, Q.entanglement_graph(9, 2))
    states = [Q.simulate(ans.circuit_for_data(x), 1 - 1e-16) for x in R.synthetic_features(2, 9, 4)]
    states += [Q.random_mps(6, [1, 2, 4, 7, 4, 2, 1], rng), Q.random_mps(2, [1, 2, 1], rng)]
    for m in states:
        T, norm = ref_pair_paulis(m.tensors)
        F, nf = ref_local_paulis(m.tensors)
        assert abs(norm - nf) < 1e-13 * nf
        assert np.abs(T[:, 1:, 0] - F[:-1]).max() < 1e-13  # T[k][p][0] = F[k][p-1]
        assert np.abs(T[:, 0, 1:] - F[1:]).max() < 1e-13  # T[k][0][q] = F[k+1][q-1]


def test_analytic_xxphase_pair_and_product_neighbour():
    """XXPhase(alpha) on |00>, theta = pi alpha / 2: cos(theta)|00> - i sin(theta)|11>.  T[X][Y] = T[Y][X] = -sin(pi alpha),
    T[Z][Z] = T[I][I] = 1, T[Z][I] = T[I][Z] = cos(pi alpha), all else 0; next to it a qubit in the product state Ry(beta)|0>
    gives the outer product of the two Pauli vectors (1, F)."""
    for alpha, beta in ((0.3, 0.25), (-0.45, 1.1), (0.0, -0.6), (0.5, 0.0)):
        gates = [("XXPhase", [0, 1], [alpha]), ("Ry", [2], [beta])]
        m = Q.simulate(Q.BoundCircuit.from_gates(3, gates), 1 - 1e-16)
        T, norm = ref_pair_paulis(m.tensors)
        s, c = math.sin(math.pi * alpha), math.cos(math.pi * alpha)
        want = np.zeros((4, 4))
        want[0, 0] = want[3, 3] = 1.0
        want[1, 2] = want[2, 1] = -s
        want[3, 0] = want[0, 3] = c
        assert np.abs(T[0] - want).max() < 1e-13
        f1 = np.array([1.0, 0.0, 0.0, c])  # qubit 1 alone: <Z> = cos(pi alpha)
        f2 = np.array([1.0, math.sin(math.pi * beta), 0.0, math.cos(math.pi * beta)])
        assert np.abs(T[1] - np.outer(f1, f2)).max() < 1e-13
        assert abs(norm - 1.0) < 1e-13


def test_pair_gram_reference_identities():
    rng = np.random.default_rng(1)
    tx = rng.uniform(-1, 1, (5, 4, 4, 4))
    K = ref_pair_gram(tx, tx, 0.25)
    assert np.allclose(np.diag(K), 1.0) and np.allclose(K, K.T)
    assert ref_pair_gram(tx, tx[:3], 0.25).shape == (3, 5)
    # ||rho - sigma||_F^2 = 1/4 sum_pq (T[p][q] - S[p][q])^2 for rho = 1/4 sum T[p][q] P_p (x) P_q, on explicit 4 x 4 matrices
    for _ in range(3):
        Tr, Ts = rng.uniform(-0.3, 0.3, (4, 4)), rng.uniform(-0.3, 0.3, (4, 4))
        Tr[0, 0] = Ts[0, 0] = 1.0
        rho = 0.25 * sum(Tr[p, q] * np.kron(PAULIS[p], PAULIS[q]) for p in range(4) for q in range(4))
        sig = 0.25 * sum(Ts[p, q] * np.kron(PAULIS[p], PAULIS[q]) for p in range(4) for q in range(4))
        assert abs(np.linalg.norm(rho - sig) ** 2 - 0.25 * np.sum((Tr - Ts) ** 2)) < 1e-14
        # and the correlators of that matrix are T again
        assert np.abs(correlators_from_rho(rho.reshape(2, 2, 2, 2)) - Tr).max() < 1e-14
    # the same identity on the states of a circuit: Frobenius distance of dense pair matrices against the correlators
    ans = Q.KernelStateAnsatz(6, 2, 1.0, Q.entanglement_graph(6, 2))
    a, b = (Q.simulate(ans.circuit_for_data(x), 1 - 1e-16) for x in R.synthetic_features(2, 6, 2))
    Ta, Tb = ref_pair_paulis(a.tensors)[0], ref_pair_paulis(b.tensors)[0]
    pa, pb = dense(a).reshape((2,) * 6), dense(b).reshape((2,) * 6)
    dist = 0.0
    for k in range(5):
        ma, mb = (np.moveaxis(p, (k, k + 1), (0, 1)).reshape(4, -1) for p in (pa, pb))
        dist += np.linalg.norm(ma @ ma.conj().T / np.vdot(pa, pa).real - mb @ mb.conj().T / np.vdot(pb, pb).real) ** 2
    assert abs(dist - 0.25 * np.sum((Ta - Tb) ** 2)) < 1e-13
    assert abs(ref_pair_gram(Ta[None], Tb[None], 0.7)[0, 0] - math.exp(-0.7 * dist)) < 1e-13


# ---- the public surface without a device ----------------------------------------------------------------------------
@pytest.mark.parametrize(
    "n_qubits,kwargs,match",
    [
        (4, {"rdm": 0}, "rdm"),
        (4, {"rdm": 3}, "rdm"),
        (4, {"rdm": "2"}, "rdm"),
        (1, {"rdm": 2}, "at least 2 qubits"),
        (4, {"rdm": 2, "pqk_gamma": 0.0}, "bandwidth"),
        (4, {"rdm": 2, "Y": np.zeros((5, 4))}, "X must not be smaller than Y"),
    ],
)
def test_build_projected_kernel_matrix_rdm_argument_errors(monkeypatch, n_qubits, kwargs, match):
    from qml_cutensornet_amd import engine
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend import kernel_state_ansatz as K

    def no_device(*a, **k):
        raise AssertionError("device work before the argument checks")

    monkeypatch.setattr(engine, "device_count", no_device)
    monkeypatch.setattr(engine, "default_context", no_device)
    ans = Q.KernelStateAnsatz(n_qubits, 1, 1.0, Q.entanglement_graph(n_qubits, 1))
    with pytest.raises(ValueError, match=match):
        K.build_projected_kernel_matrix(SingleComm(), ans, np.zeros((3, n_qubits)), truncation_error=1e-16, **kwargs)


def test_projected_pair_gram_shape_checks_need_no_device():
    from qml_cutensornet_amd import engine

    ctx = engine.Context.__new__(engine.Context)  # the checks come before the handle is touched
    for bad in (np.zeros((3, 4, 3)), np.zeros((3, 0, 4, 4)), np.zeros((3, 2, 4, 3))):
        with pytest.raises(ValueError, match="features"):
            engine.Context.projected_pair_gram(ctx, bad)
    with pytest.raises(ValueError, match="do not match"):
        engine.Context.projected_pair_gram(ctx, np.zeros((3, 2, 4, 4)), np.zeros((2, 3, 4, 4)))
    with pytest.raises(ValueError, match="bandwidth"):
        engine.Context.projected_pair_gram(ctx, np.zeros((3, 2, 4, 4)), gamma=-1.0)


def test_library_exports_pair_entry_points(built):
    from qml_cutensornet_amd import engine

    L = engine.lib()
    for name in ("qk_local_pair_paulis_host", "qk_projected_pair_gram_host"):
        assert name in engine.EXPORTED_SYMBOLS
        assert hasattr(L, name)
