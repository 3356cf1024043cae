"""Windows of k qubits on the host (no GPU): ``MPS.window_rdm`` -- the numpy mirror of qk_window_rdms_host -- against dense state
vectors of a general-gauge chain, ``engine.rdm_paulis`` / ``paulis_rdm``, ``engine.window_overlaps`` against ``MPS.block_overlap``
at both ends, the purities against the bond spectra, the argument checks of ``build_projected_kernel_matrix(rdm >= 3)`` (raised
before any device work) and the library's export."""
import itertools

import numpy as np
import pytest

import qml_cutensornet_amd as Q
from helpers import scrambled
from qml_cutensornet_amd import engine
from test_projected_host import dense, ref_local_paulis

N = 8
BONDS = [1, 2, 4, 7, 9, 7, 4, 2, 1]
WINDOWS = [(a, w) for w in range(1, 7) for a in range(N - w + 1)]
PAULI = np.array([[[1, 0], [0, 1]], [[0, 1], [1, 0]], [[0, -1j], [1j, 0]], [[1, 0], [0, -1]]], dtype=complex)


@pytest.fixture(scope="module")
def chain():
    rng = np.random.default_rng(8)
    return scrambled(Q.random_mps(N, BONDS, rng), rng, scale=3.7)


@pytest.fixture(scope="module")
def chain2():
    rng = np.random.default_rng(9)
    return scrambled(Q.random_mps(N, BONDS, rng), rng, scale=0.6)


def dense_window(psi, n, a, w):
    """rho of the qubits a .. a+w-1 of a dense vector (qubit 0 = most significant axis), qubit a the most significant bit."""
    t = np.asarray(psi).reshape(2**a, 2**w, -1)
    return np.einsum("lsr,ltr->st", t, t.conj()) / float(np.vdot(psi, psi).real)


def test_window_rdm_against_dense(chain):
    psi = dense(chain)
    assert abs(np.vdot(psi, psi).real - 1.0) > 1.0  # not normalised: the scale is part of the test
    worst = 0.0
    for a, w in WINDOWS:
        rho = chain.window_rdm(a, w)
        assert rho.shape == (2**w, 2**w) and rho.dtype == np.complex128
        worst = max(worst, float(np.abs(rho - dense_window(psi, N, a, w)).max()))
        assert abs(np.trace(rho) - 1.0) < 1e-14
    assert worst < 1e-14, worst


def test_window_rdm_arguments(chain):
    for a, w in ((0, 0), (0, 7), (-1, 2), (7, 2), (3, 6)):
        with pytest.raises(ValueError):
            chain.window_rdm(a, w)
    with pytest.raises(ValueError):
        chain.window_rdm(0.0, 2)
    with pytest.raises(ValueError):
        chain.window_rdm(0, True)


def test_width_one_is_the_bloch_formula(chain):
    F, _ = ref_local_paulis([np.asarray(t) for t in chain.tensors])
    for a in range(N):
        rho = chain.window_rdm(a, 1)
        want = 0.5 * (PAULI[0] + F[a, 0] * PAULI[1] + F[a, 1] * PAULI[2] + F[a, 2] * PAULI[3])
        assert np.abs(rho - want).max() < 1e-14
        assert np.abs(engine.rdm_paulis(rho) - np.concatenate([[1.0], F[a]])).max() < 1e-14


def test_tracing_out_the_last_qubit(chain):
    for a, w in WINDOWS:
        if w >= 2:
            rho = chain.window_rdm(a, w).reshape(2 ** (w - 1), 2, 2 ** (w - 1), 2)
            assert np.abs(np.einsum("sutu->st", rho) - chain.window_rdm(a, w - 1)).max() < 1e-14


def test_paulis_round_trip_and_convention(chain):
    rng = np.random.default_rng(2)
    for w in range(1, 5):
        rho = np.stack([chain.window_rdm(a, w) for a in range(N - w + 1)])
        c = engine.rdm_paulis(rho)
        assert c.shape == (N - w + 1,) + (4,) * w and c.dtype == np.float64
        assert np.abs(c[(slice(None),) + (0,) * w] - 1.0).max() < 1e-14  # the all-identity coefficient is the trace
        assert np.abs(engine.paulis_rdm(c, width=w) - rho).max() < 1e-15
        # c[p_0 .. p_{w-1}] = tr(rho P_{p_0} (x) .. (x) P_{p_{w-1}}) on a few strings, qubit a of the window first
        for _ in range(6):
            p = tuple(int(v) for v in rng.integers(0, 4, w))
            op = np.ones((1, 1), dtype=complex)
            for q in p:
                op = np.kron(op, PAULI[q])
            for a in range(N - w + 1):
                assert abs(np.trace(rho[a] @ op) - c[(a,) + p]) < 1e-14
    # random real coefficients, the other way round; a leading axis of size 4 needs the width
    c = rng.standard_normal((4, 3, 4, 4, 4))
    assert np.abs(engine.rdm_paulis(engine.paulis_rdm(c, width=3)) - c).max() < 1e-14
    assert engine.paulis_rdm(c[0]).shape == (3, 8, 8)
    with pytest.raises(ValueError):
        engine.paulis_rdm(np.zeros((3, 5)))
    with pytest.raises(ValueError):
        engine.rdm_paulis(np.zeros((3, 3)))


def test_width_two_is_the_pair_convention(chain):
    """T[k][p][q] = <P_p on k, P_q on k+1> from the dense vector, written out with kron."""
    psi = dense(chain)
    for a in (0, 3, 6):
        c = engine.rdm_paulis(chain.window_rdm(a, 2))
        rho = dense_window(psi, N, a, 2)
        for p, q in itertools.product(range(4), repeat=2):
            assert abs(np.trace(rho @ np.kron(PAULI[p], PAULI[q])).real - c[p, q]) < 1e-14


def all_windows(m, w):
    return np.stack([m.window_rdm(a, w) for a in range(len(m) - w + 1)])


def test_window_overlaps_against_block_overlap(chain, chain2):
    states = [chain, chain2]
    for w in range(1, 7):
        rx = np.stack([all_windows(m, w) for m in states])
        O, Sx, Sy = engine.window_overlaps(rx)
        nw = N - w + 1
        assert O.shape == (nw, 2, 2) and Sx.shape == (nw, 2) and Sy is Sx
        assert np.array_equal(O, O.transpose(0, 2, 1)) and np.array_equal(O[:, [0, 1], [0, 1]], Sx)
        for i, j in ((0, 0), (0, 1), (1, 1)):
            assert abs(O[0, j, i] - states[i].block_overlap(states[j], w, "left")) < 1e-13
            assert abs(O[nw - 1, j, i] - states[i].block_overlap(states[j], w, "right")) < 1e-13
        # the rectangular form: rows are Y
        O2, S2x, S2y = engine.window_overlaps(rx[:1], rx)
        assert O2.shape == (nw, 2, 1) and np.abs(O2[:, :, 0] - O[:, :, 0]).max() < 1e-15
        assert np.abs(S2x - Sx[:, :1]).max() < 1e-15 and np.abs(S2y - Sx).max() < 1e-15
        K = engine.block_kernel(O[1], Sx[1], form="rbf", gamma=0.7)
        d = rx[0, 1] - rx[1, 1]
        assert abs(K[1, 0] - np.exp(-0.7 * float((np.abs(d) ** 2).sum()))) < 1e-14


def test_purity_against_bond_spectra(chain):
    spectra = chain.bond_spectra()
    for w in range(1, 7):
        _, S, _ = engine.window_overlaps(all_windows(chain, w)[None])
        assert abs(S[0, 0] - float((spectra[w - 1] ** 2).sum())) < 1e-13
        assert abs(S[N - w, 0] - float((spectra[N - w - 1] ** 2).sum())) < 1e-13


def test_window_columns_and_shapes(chain):
    r = np.stack([all_windows(chain, 2)])
    f = engine.window_columns(r)
    assert f.shape == (1, 2 * 7 * 16) and np.array_equal(f[0, :112], r.real.reshape(-1)) and np.array_equal(f[0, 112:], r.imag.reshape(-1))
    for bad in (np.zeros((2, 3, 3, 3)), np.zeros((2, 4, 4)), np.zeros((2, 0, 4, 4))):
        with pytest.raises(ValueError):
            engine.window_overlaps(bad)
    with pytest.raises(ValueError):
        engine.window_overlaps(r, np.zeros((1, 7, 8, 8)))


def test_builder_argument_checks():
    """rdm >= 3 with window=True is the window form: the cases it does not take are rejected before any device work, and rdm >= 3
    without the switch stays the error it was."""
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend import kernel_state_ansatz as G

    n = 6
    ans = Q.KernelStateAnsatz(n, 1, 1.0, Q.entanglement_graph(n, 1))
    X = np.linspace(0.1, 0.9, 2 * n).reshape(2, n)
    for kw in (dict(rdm=3, pair_distance=2), dict(rdm=3, shots=10), dict(rdm=3, observables=["ZZ"]), dict(rdm=7), dict(rdm=0), dict(rdm=1), dict(rdm=2),
               dict(rdm=True), dict(rdm=3.0)):
        with pytest.raises(ValueError):
            G.build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, window=True, **kw)
    with pytest.raises(ValueError, match="window=True"):
        G.build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, rdm=3)
    with pytest.raises(ValueError, match="window must be"):
        G.build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, rdm=3, window=1)
    ans4 = Q.KernelStateAnsatz(4, 1, 1.0, Q.entanglement_graph(4, 1))
    with pytest.raises(ValueError):
        G.build_projected_kernel_matrix(SingleComm(), ans4, X[:, :4], truncation_error=1e-16, rdm=5, window=True)


def test_exported():
    assert "qk_window_rdms_host" in engine.EXPORTED_SYMBOLS
    import os

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qkgram.h")).read()
    assert "int qk_window_rdms_host(" in header
