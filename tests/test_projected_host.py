"""Projected quantum kernel on the host (no GPU): the numpy reference of the local sweep (one-qubit reduced density matrices
from left and right environments) against dense-state-vector partial traces, analytic Bloch vectors of product circuits,
the argument checks of ``build_projected_kernel_matrix`` (raised before any device work) and the library's exports."""
import math

import numpy as np
import pytest

import qml_cutensornet_amd as Q
from oracle import restatement as R


# ---- numpy reference (the contract of qk_local_paulis_host) -----------------------------------------------------------
def ref_local_paulis(tensors):
    """Bloch vectors F[k] = (<X_k>, <Y_k>, <Z_k>) and <psi|psi> of an MPS given as [chi_k][2][chi_k+1] complex tensors."""
    n = len(tensors)
    Rs = [None] * (n + 1)
    Rs[n] = np.ones((1, 1), dtype=complex)
    for k in range(n - 1, -1, -1):
        A = tensors[k]
        Rs[k] = np.einsum("lsr,rq,msq->lm", A, Rs[k + 1], A.conj(), optimize=True)
    norm = Rs[0][0, 0].real
    L = np.ones((1, 1), dtype=complex)
    F = np.zeros((n, 3))
    for k in range(n):
        A = tensors[k]
        rho = np.einsum("lm,lsr,rq,mtq->st", L, A, Rs[k + 1], A.conj(), optimize=True) / norm
        F[k] = (2 * rho[0, 1].real, -2 * rho[0, 1].imag, (rho[0, 0] - rho[1, 1]).real)
        L = np.einsum("lm,lsr,msq->rq", L, A, A.conj(), optimize=True)
    return F, norm


def bloch_from_dense(psi, n):
    """Bloch vectors of every qubit of a dense state (qubit 0 = most significant axis) by partial traces."""
    psi = np.asarray(psi).reshape((2,) * n)
    norm = float(np.vdot(psi, psi).real)
    F = np.zeros((n, 3))
    for k in range(n):
        m = np.moveaxis(psi, k, 0).reshape(2, -1)
        rho = m @ m.conj().T / norm
        F[k] = (2 * rho[0, 1].real, -2 * rho[0, 1].imag, (rho[0, 0] - rho[1, 1]).real)
    return F, norm


def ref_projected_gram(fx, fy, g):
    """K[j, i] = exp(-g/2 sum_k |fx[i, k] - fy[j, k]|^2)."""
    d = fx[None, :, :, :] - fy[:, None, :, :]
    return np.exp(-0.5 * g * (d * d).sum(axis=(2, 3)))


def dense(mps):
    v = np.ones((1, 1), dtype=complex)
    for t in mps.tensors:
        v = np.tensordot(v, t, axes=(v.ndim - 1, 0))
    return v.reshape(-1)


def zz_template(n):
    """A Havlicek-style feature map of Rx, Ry and ZZPhase on a ring of neighbours."""
    gates = [("H", [q], None) for q in range(n)]
    for q in range(n):
        gates.append(("Ry", [q], (0.7, (q % n, 0.3, 1.0))))
        gates.append(("Rx", [q], (0.4, ((q + 1) % n, 1.0, -0.5))))
    for q in range(n - 1):
        gates.append(("ZZPhase", [q, q + 1], (0.8, (q, math.pi, -1.0), (q + 1, math.pi, -1.0))))
    gates.append(("ZZPhase", [0, n - 1], (0.5, (0, 1.0, 0.5), (n - 1, 1.0, 0.5))))
    for q in range(n):
        gates.append(("Ry", [q], (0.3, (q, 0.0, 1.0))))
    return gates


# ---- the reference against partial traces -------------------------------------------------------------------------
@pytest.mark.parametrize("n,reps,d", [(8, 2, 1), (10, 2, 2), (12, 1, 3)])
def test_reference_matches_partial_trace_kernel_state_ansatz(n, reps, d):
    ans = Q.KernelStateAnsatz(n, reps, 1.0, Q.entanglement_graph(n, d))
    X = R.synthetic_features(3, n, 11 + n)
    for x in X:
        m = Q.simulate(ans.circuit_for_data(x), 1 - 1e-16)
        F, norm = ref_local_paulis(m.tensors)
        Fd, nd = bloch_from_dense(dense(m), n)
        assert np.abs(F - Fd).max() < 1e-13
        assert abs(norm - nd) < 1e-13 * nd


@pytest.mark.parametrize("n", [8, 11])
def test_reference_matches_partial_trace_circuit_ansatz(n):
    ca = Q.CircuitAnsatz(n, zz_template(n))
    X = R.synthetic_features(3, n, 5)
    for x in X:
        m = Q.simulate(ca.circuit_for_data(x), 1 - 1e-16)
        F, _ = ref_local_paulis(m.tensors)
        Fd, _ = bloch_from_dense(dense(m), n)
        assert np.abs(F - Fd).max() < 1e-13


def test_reference_ragged_random_and_unnormalised():
    rng = np.random.default_rng(7)
    for prof in ([1, 2, 4, 8, 13, 9, 5, 3, 2, 1], [1, 2, 3, 6, 11, 7, 4, 2, 1], [1, 1], [1, 2, 1]):
        m = Q.random_mps(len(prof) - 1, prof, rng)
        F, norm = ref_local_paulis(m.tensors)
        Fd, nd = bloch_from_dense(dense(m), len(prof) - 1)
        assert np.abs(F - Fd).max() < 1e-13 and abs(norm - nd) < 1e-13
        scaled = [t * (3.7 if k == 0 else 1.0) for k, t in enumerate(m.tensors)]
        Fs, ns = ref_local_paulis(scaled)
        assert np.abs(Fs - Fd).max() < 1e-13
        assert abs(ns - 3.7**2 * nd) < 1e-12 * ns


def test_analytic_bloch_vectors_of_product_circuits():
    alphas = [0.0, 0.25, -0.6, 1.3]
    n = 3 * len(alphas) + 1
    gates, want = [], np.zeros((n, 3))
    for k, a in enumerate(alphas):
        gates.append(("Ry", [k], [a]))
        want[k] = (math.sin(math.pi * a), 0.0, math.cos(math.pi * a))
        q = len(alphas) + k
        gates.append(("Rx", [q], [a]))
        want[q] = (0.0, -math.sin(math.pi * a), math.cos(math.pi * a))
    for q in range(2 * len(alphas), n - 1):
        gates.append(("H", [q], []))
        want[q] = (1.0, 0.0, 0.0)
    want[n - 1] = (0.0, 0.0, 1.0)  # |0>
    m = Q.simulate(Q.BoundCircuit.from_gates(n, gates), 1 - 1e-16)
    F, norm = ref_local_paulis(m.tensors)
    assert np.abs(F - want).max() < 1e-13
    assert abs(norm - 1.0) < 1e-13


def test_projected_gram_reference_identities():
    rng = np.random.default_rng(1)
    fx = rng.uniform(-1, 1, (5, 4, 3))
    K = ref_projected_gram(fx, fx, 0.25)
    assert np.allclose(np.diag(K), 1.0) and np.allclose(K, K.T)
    # ||rho - sigma||_F^2 = |r - s|^2 / 2 for one-qubit density matrices with Bloch vectors r, s
    paulis = [np.array([[0, 1], [1, 0]]), np.array([[0, -1j], [1j, 0]]), np.diag([1.0, -1.0])]
    r, s = rng.uniform(-0.5, 0.5, 3), rng.uniform(-0.5, 0.5, 3)
    rho = 0.5 * (np.eye(2) + sum(c * p for c, p in zip(r, paulis)))
    sig = 0.5 * (np.eye(2) + sum(c * p for c, p in zip(s, paulis)))
    assert abs(np.linalg.norm(rho - sig) ** 2 - 0.5 * np.sum((r - s) ** 2)) < 1e-15


# ---- the public surface without a device ----------------------------------------------------------------------------
@pytest.mark.parametrize(
    "kwargs,match",
    [
        ({"Y": np.zeros((5, 4)), "truncation_error": 1e-16}, "X must not be smaller than Y"),
        ({"truncation_error": None}, "truncation error"),
        ({"truncation_error": 1e-16, "pqk_gamma": 0.0}, "bandwidth"),
        ({"truncation_error": 1e-16, "pqk_gamma": -1.0}, "bandwidth"),
        ({"truncation_error": 1e-16, "pqk_gamma": float("nan")}, "bandwidth"),
    ],
)
def test_build_projected_kernel_matrix_argument_errors(monkeypatch, kwargs, match):
    from qml_cutensornet_amd import engine
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend import kernel_state_ansatz as K

    def no_device(*a, **k):
        raise AssertionError("device work before the argument checks")

    monkeypatch.setattr(engine, "device_count", no_device)
    monkeypatch.setattr(engine, "default_context", no_device)
    ans = Q.KernelStateAnsatz(4, 1, 1.0, Q.entanglement_graph(4, 1))
    with pytest.raises(ValueError, match=match):
        K.build_projected_kernel_matrix(SingleComm(), ans, np.zeros((3, 4)), **kwargs)


def test_projected_gamma_default_and_checks():
    from qml_cutensornet_amd import engine

    assert engine.projected_gamma(None, 8) == 0.125
    assert engine.projected_gamma(0.3, 8) == 0.3
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            engine.projected_gamma(bad, 8)


def test_library_exports_projected_entry_points(built):
    from qml_cutensornet_amd import engine

    L = engine.lib()
    for name in ("qk_local_paulis_host", "qk_projected_gram_host"):
        assert name in engine.EXPORTED_SYMBOLS
        assert hasattr(L, name)
