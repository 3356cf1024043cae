"""Two-qubit projected quantum kernel over pairs up to a chosen distance, on the host (no GPU): the numpy reference of the
distance sweep (the four open left environments of qubit k carried across the sites between k and k+d, closed with the open
right environment of qubit k+d) against dense-state-vector partial traces and against the neighbour reference, an analytic
XXPhase case on qubits (0, 2), ``engine.pair_table``, the shape inference of ``projected_pair_gram(max_dist=...)``, the
``pair_distance`` argument checks of ``build_projected_kernel_matrix`` (raised before any device work) and the library's
exports."""
import math

import numpy as np
import pytest

import qml_cutensornet_amd as Q
from oracle import restatement as R
from qml_cutensornet_amd import engine
from test_projected_host import dense
from test_projected_pair_host import correlators_from_rho, ref_pair_paulis


# ---- numpy reference (the contract of qk_local_pair_paulis_dist_host) --------------------------------------------------
def pair_index(n, d, k):
    """Row of the pair (k, k + d): distance-major, sum_{e=1}^{d-1} (n - e) + k."""
    return (d - 1) * n - (d - 1) * d // 2 + k


def ref_pair_paulis_dist(tensors, max_dist):
    """Pauli correlators T[index(d, k)][p][q] = <P_p on k, P_q on k+d>, d = 1 .. max_dist, and <psi|psi> of an MPS given as
    [chi_k][2][chi_k+1] complex tensors.  E_{k->k+1}[s][s'] = W_{k,s}[.][(s', .)]; across a site m between the two qubits
    E_{k->m+1} = sum_u A_m^u^T E_{k->m} conj(A_m^u); rho_{k,j} = sum E_{k->j}[s][s'][b][a] V_{j,t}[b][(t', a)]."""
    n, D = len(tensors), int(max_dist)
    assert 1 <= D <= n - 1
    Rs = [None] * (n + 1)
    Rs[n] = np.ones((1, 1), dtype=complex)
    for k in range(n - 1, -1, -1):
        A = tensors[k]
        Rs[k] = np.einsum("lsr,rq,msq->lm", A, Rs[k + 1], A.conj(), optimize=True)
    norm = Rs[0][0, 0].real
    T = np.zeros((D * n - D * (D + 1) // 2, 4, 4))
    L = np.ones((1, 1), dtype=complex)
    window = {}  # origin k -> E_{k->j}[s][b][s'][a] at the current bond j
    for j in range(n):
        A = tensors[j]
        if window:
            V = np.einsum("rtc,qvd,cd->trvq", A, A.conj(), Rs[j + 1], optimize=True)  # V[t][b][t'][a]
            for k, E in window.items():
                rho = np.einsum("sruq,trvq->stuv", E, V, optimize=True) / norm
                row = pair_index(n, j - k, k)
                T[row] = correlators_from_rho(rho)
                T[row, 0, 0] = 1.0
        window = {k: np.einsum("sbua,bvc,avd->scud", E, A, A.conj(), optimize=True) for k, E in window.items() if j + 1 - k <= D}
        window[j] = np.einsum("lm,lsr,muq->sruq", L, A, A.conj(), optimize=True)  # W[s][b'][s'][a']
        L = np.einsum("lm,lsr,msq->rq", L, A, A.conj(), optimize=True)
    return T, norm


def pair_dist_from_dense(psi, n, max_dist):
    """T[index(d, k)][p][q] of every pair up to max_dist of a dense state (qubit 0 = most significant axis) by partial traces."""
    psi = np.asarray(psi).reshape((2,) * n)
    norm = float(np.vdot(psi, psi).real)
    D = int(max_dist)
    T = np.zeros((D * n - D * (D + 1) // 2, 4, 4))
    for d in range(1, D + 1):
        for k in range(n - d):
            m = np.moveaxis(psi, (k, k + d), (0, 1)).reshape(4, -1)
            T[pair_index(n, d, k)] = correlators_from_rho((m @ m.conj().T / norm).reshape(2, 2, 2, 2))
    return T, norm


def _check_state(m, n, D):
    T, norm = ref_pair_paulis_dist(m.tensors, D)
    Td, nd = pair_dist_from_dense(dense(m), n, D)
    err = np.abs(T - Td).max()
    assert err < 1e-13, err
    assert abs(norm - nd) < 1e-13 * nd
    assert np.all(T[:, 0, 0] == 1.0)
    # the distance-1 block is the neighbour reference
    assert np.abs(T[: n - 1] - ref_pair_paulis(m.tensors)[0]).max() < 1e-13
    return T


# ---- the reference against partial traces and the neighbour reference --------------------------------------------------
@pytest.mark.parametrize("n,reps,d,D", [(8, 2, 1, 3), (10, 2, 2, 2), (12, 1, 3, 4), (6, 2, 2, 5)])
def test_dist_reference_matches_partial_trace_kernel_state_ansatz(n, reps, d, D):
    ans = Q.KernelStateAnsatz(n, reps, 1.0, Q.entanglement_graph(n, d))
    for x in R.synthetic_features(3, n, 11 + n):
        _check_state(Q.simulate(ans.circuit_for_data(x), 1 - 1e-16), n, D)


def test_dist_reference_ragged_random_and_unnormalised():
    rng = np.random.default_rng(7)
    for prof in ([1, 2, 4, 8, 13, 9, 5, 3, 2, 1], [1, 2, 3, 6, 11, 7, 4, 2, 1], [1, 2, 1], [1, 1, 1], [1, 2, 2, 1]):
        n = len(prof) - 1
        m = Q.random_mps(n, prof, rng)
        T = _check_state(m, n, n - 1)
        scaled = [t * (3.7 if k == min(1, n - 1) else 1.0) for k, t in enumerate(m.tensors)]
        Ts, ns = ref_pair_paulis_dist(scaled, n - 1)
        assert np.abs(Ts - T).max() < 1e-13
        assert abs(ns - 3.7**2 * ref_pair_paulis_dist(m.tensors, n - 1)[1]) < 1e-12 * ns


def test_dist_block_one_is_the_neighbour_reference_for_every_distance():
    rng = np.random.default_rng(5)
    m = Q.random_mps(7, [1, 2, 4, 7, 6, 4, 2, 1], rng)
    Tn = ref_pair_paulis(m.tensors)[0]
    for D in range(1, 7):
        T = ref_pair_paulis_dist(m.tensors, D)[0]
        assert T.shape == (D * 7 - D * (D + 1) // 2, 4, 4)
        assert np.abs(T[:6] - Tn).max() < 1e-13
        # a smaller D is a prefix of a larger one: the order is distance-major
        assert np.abs(T - ref_pair_paulis_dist(m.tensors, 6)[0][: len(T)]).max() < 1e-13


def test_analytic_xxphase_on_qubits_0_and_2():
    """XXPhase(alpha) on qubits (0, 2) of |000>: T[X][Y] = T[Y][X] = -sin(pi alpha), T[Z][I] = T[I][Z] = cos(pi alpha),
    T[Z][Z] = T[I][I] = 1 on the pair (0, 2), all else 0; qubit 1 stays |0>, so the neighbouring pairs are outer products."""
    for alpha in (0.3, -0.45, 0.0, 0.5):
        m = Q.simulate(Q.BoundCircuit.from_gates(3, [("XXPhase", [0, 2], [alpha])]), 1 - 1e-16)
        T, norm = ref_pair_paulis_dist(m.tensors, 2)
        s, c = math.sin(math.pi * alpha), math.cos(math.pi * alpha)
        want = np.zeros((4, 4))
        want[0, 0] = want[3, 3] = 1.0
        want[1, 2] = want[2, 1] = -s
        want[3, 0] = want[0, 3] = c
        assert T.shape == (3, 4, 4)
        assert np.abs(T[pair_index(3, 2, 0)] - want).max() < 1e-13
        edge, mid = np.array([1.0, 0.0, 0.0, c]), np.array([1.0, 0.0, 0.0, 1.0])
        assert np.abs(T[0] - np.outer(edge, mid)).max() < 1e-13
        assert np.abs(T[1] - np.outer(mid, edge)).max() < 1e-13
        assert abs(norm - 1.0) < 1e-13


# ---- the public surface without a device ----------------------------------------------------------------------------
def test_pair_table_order_and_count():
    for n, D in ((2, 1), (5, 1), (5, 3), (9, 8), (12, 2)):
        tab = engine.pair_table(n, D)
        assert tab.shape == (D * n - D * (D + 1) // 2, 2) and np.issubdtype(tab.dtype, np.integer)
        want = [(k, k + d) for d in range(1, D + 1) for k in range(n - d)]
        assert [tuple(r) for r in tab.tolist()] == want
        for row, (a, b) in enumerate(want):
            assert pair_index(n, b - a, a) == row
    assert engine.pair_table(4, 1).tolist() == [[0, 1], [1, 2], [2, 3]]
    assert engine.pair_table(4, 2).tolist() == [[0, 1], [1, 2], [2, 3], [0, 2], [1, 3]]
    assert engine.pair_table(6).tolist() == engine.pair_table(6, 1).tolist()
    for n, D in ((4, 0), (4, 4), (1, 1)):
        with pytest.raises(ValueError, match="max_dist"):
            engine.pair_table(n, D)
    # the distance of an entanglement map: the pairs its gates touch are rows of the table
    pairs = Q.entanglement_graph(7, 3)
    D = max(abs(a - b) for a, b in pairs)
    assert D == 3
    rows = {tuple(r) for r in engine.pair_table(7, D).tolist()}
    assert {tuple(sorted(p)) for p in pairs} <= rows


class _FakeLib:
    """Stands in for the library: records the arguments of the Gram calls and does nothing."""

    def __init__(self):
        self.calls = []

    def qk_projected_pair_gram_host(self, h, n, nx, tx, ny, ty, g, out, ld):
        self.calls.append(("pair", n, 1, nx, ny, g))
        return 0

    def qk_projected_pair_gram_dist_host(self, h, n, D, nx, tx, ny, ty, g, out, ld):
        self.calls.append(("dist", n, D, nx, ny, g))
        return 0


def test_projected_pair_gram_max_dist_shape_inference_needs_no_device(monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(engine, "lib", lambda: fake)
    ctx = engine.Context.__new__(engine.Context)  # the checks come before the handle is touched
    ctx._h = None
    # n_pairs = D n - D (D + 1) / 2: (n, D) = (4, 2) -> 5, (12, 2) -> 21, (14, 3) -> 36, (6, 5) -> 15
    for n, D in ((4, 2), (12, 2), (14, 3), (6, 5), (3, 2)):
        n_pairs = D * n - D * (D + 1) // 2
        K = engine.Context.projected_pair_gram(ctx, np.zeros((3, n_pairs, 4, 4)), max_dist=D)
        assert K.shape == (3, 3)
        assert fake.calls[-1] == ("dist", n, D, 3, 3, 1.0 / (n * D))  # the default bandwidth 1 / (n_qubits D)
    engine.Context.projected_pair_gram(ctx, np.zeros((3, 5, 4, 4)), np.zeros((2, 5, 4, 4)), gamma=0.3, max_dist=2)
    assert fake.calls[-1] == ("dist", 4, 2, 3, 2, 0.3)
    # max_dist = 1 stays the neighbour call with its default 1 / n_sites
    engine.Context.projected_pair_gram(ctx, np.zeros((3, 5, 4, 4)))
    assert fake.calls[-1] == ("pair", 6, 1, 3, 3, 1.0 / 6)
    # no chain with n_sites >= max_dist + 1 has that many pairs
    for shape, D in (((3, 4, 4, 4), 2), ((3, 1, 4, 4), 2), ((3, 5, 4, 4), 3), ((3, 6, 4, 4), 4), ((3, 5, 4, 4), 0), ((3, 5, 4, 4), -2)):
        with pytest.raises(ValueError, match="features"):
            engine.Context.projected_pair_gram(ctx, np.zeros(shape), max_dist=D)
    for bad in (np.zeros((3, 4, 3)), np.zeros((3, 0, 4, 4)), np.zeros((3, 5, 4, 3))):
        with pytest.raises(ValueError, match="features"):
            engine.Context.projected_pair_gram(ctx, bad, max_dist=2)
    with pytest.raises(ValueError, match="do not match"):
        engine.Context.projected_pair_gram(ctx, np.zeros((3, 5, 4, 4)), np.zeros((2, 7, 4, 4)), max_dist=2)
    with pytest.raises(ValueError, match="bandwidth"):
        engine.Context.projected_pair_gram(ctx, np.zeros((3, 5, 4, 4)), gamma=-1.0, max_dist=2)


@pytest.mark.parametrize(
    "n_qubits,kwargs",
    [
        (4, {"rdm": 2, "pair_distance": 0}),
        (4, {"rdm": 2, "pair_distance": -1}),
        (4, {"rdm": 2, "pair_distance": 4}),
        (4, {"rdm": 2, "pair_distance": 2.0}),
        (4, {"rdm": 2, "pair_distance": "2"}),
        (4, {"rdm": 2, "pair_distance": None}),
        (4, {"rdm": 1, "pair_distance": 2}),
        (4, {"pair_distance": 3}),
        (2, {"rdm": 2, "pair_distance": 2}),
    ],
)
def test_build_projected_kernel_matrix_pair_distance_argument_errors(monkeypatch, n_qubits, kwargs):
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend import kernel_state_ansatz as K

    def no_device(*a, **k):
        raise AssertionError("device work before the argument checks")

    monkeypatch.setattr(engine, "device_count", no_device)
    monkeypatch.setattr(engine, "default_context", no_device)
    ans = Q.KernelStateAnsatz(n_qubits, 1, 1.0, Q.entanglement_graph(n_qubits, 1))
    with pytest.raises(ValueError, match="pair_distance"):
        K.build_projected_kernel_matrix(SingleComm(), ans, np.zeros((3, n_qubits)), truncation_error=1e-16, **kwargs)


def test_library_exports_dist_entry_points(built):
    L = engine.lib()
    for name in ("qk_local_pair_paulis_dist_host", "qk_projected_pair_gram_dist_host"):
        assert name in engine.EXPORTED_SYMBOLS
        assert hasattr(L, name)
