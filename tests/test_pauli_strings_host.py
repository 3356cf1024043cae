"""Pauli-string expectation values on the host (no GPU): the numpy reference of qk_pauli_strings_host (a left environment, one
transfer step per site of the support with the Pauli on the ket index, a right environment) against dense state vectors, against
the merged references (Bloch vectors, pair correlators up to a distance) and analytic cases; ``engine.pauli_strings``, the
``observables`` argument checks of ``build_projected_kernel_matrix`` (raised before any device work) and the library's exports."""
import math

import numpy as np
import pytest

import qml_cutensornet_amd as Q
from oracle import restatement as R
from qml_cutensornet_amd import engine
from test_projected_dist_host import ref_pair_paulis_dist
from test_projected_host import dense, ref_local_paulis

PAULI = np.array([[[1, 0], [0, 1]], [[0, 1], [1, 0]], [[0, -1j], [1j, 0]], [[1, 0], [0, -1]]], dtype=complex)  # P[code][s'][s]


# ---- numpy reference (the contract of qk_pauli_strings_host) ----------------------------------------------------------
def ref_pauli_strings(tensors, strings):
    """values[m] = <psi|P_m|psi> / <psi|psi> and <psi|psi> of an MPS given as [chi_k][2][chi_k+1] complex tensors; strings is an
    integer array (m, n) of codes 0..3.  E_a = L_a, E_{k+1} = einsum("lm,lsr,muq,us->rq", E_k, A_k, conj(A_k), P_c[k]) for k in
    the support [a, b], value = sum E_{b+1} R_{b+1} / L_n; the imaginary part is dropped; an all-identity string is exactly 1."""
    n = len(tensors)
    strings = np.asarray(strings)
    assert strings.ndim == 2 and strings.shape[1] == n
    Rs = [None] * (n + 1)
    Rs[n] = np.ones((1, 1), dtype=complex)
    for k in range(n - 1, -1, -1):
        Rs[k] = np.einsum("lsr,rq,msq->lm", tensors[k], Rs[k + 1], tensors[k].conj(), optimize=True)
    Ls = [np.ones((1, 1), dtype=complex)]
    for k in range(n):
        Ls.append(np.einsum("lm,lsr,msq->rq", Ls[k], tensors[k], tensors[k].conj(), optimize=True))
    norm = Ls[n][0, 0].real
    vals = np.ones(len(strings))
    for m, c in enumerate(strings):
        nz = np.flatnonzero(c)
        if nz.size == 0:
            continue
        a, b = int(nz[0]), int(nz[-1])
        E = Ls[a]
        for k in range(a, b + 1):
            E = np.einsum("lm,lsr,muq,us->rq", E, tensors[k], tensors[k].conj(), PAULI[c[k]], optimize=True)
        vals[m] = (E * Rs[b + 1]).sum().real / norm
    return vals, norm


def pauli_strings_from_dense(psi, n, strings):
    """The same values from a dense state (qubit 0 = most significant axis): <psi|P|psi> / <psi|psi>."""
    psi = np.asarray(psi).reshape((2,) * n)
    norm = float(np.vdot(psi, psi).real)
    vals = np.ones(len(strings))
    for m, c in enumerate(np.asarray(strings)):
        if not np.any(c):
            continue
        phi = psi
        for k in np.flatnonzero(c):
            phi = np.moveaxis(np.tensordot(PAULI[c[k]], phi, axes=(1, k)), 0, k)
        vals[m] = np.vdot(psi, phi).real / norm
    return vals, norm


def sparse_strings(n, count, rng):
    """Sparse strings: weight 1..4 inside a window of min(6, n) sites at a random position, random non-identity codes."""
    S = np.zeros((count, n), dtype=np.uint8)
    w = min(6, n)
    for row in S:
        start = rng.integers(0, n - w + 1)
        sites = start + rng.choice(w, size=rng.integers(1, min(4, w) + 1), replace=False)
        row[sites] = rng.integers(1, 4, size=len(sites))
    return S


def weight_one_strings(n):
    """The 3 n strings P_c on qubit k, row 3 k + (c - 1): the columns of ``ref_local_paulis``'s F, flattened."""
    S = np.zeros((3 * n, n), dtype=np.uint8)
    for k in range(n):
        for c in (1, 2, 3):
            S[3 * k + c - 1, k] = c
    return S


def pair_strings(n, D):
    """The 16 n_pairs strings (P_p on k, P_q on k+d), row 16 pair + 4 p + q in ``engine.pair_table(n, D)`` order."""
    tab = engine.pair_table(n, D)
    S = np.zeros((16 * len(tab), n), dtype=np.uint8)
    for row, (a, b) in enumerate(tab):
        for p in range(4):
            for q in range(4):
                S[16 * row + 4 * p + q, a], S[16 * row + 4 * p + q, b] = p, q
    return S


def _strings_for(n, rng, count=24):
    full = np.vstack([rng.integers(1, 4, size=(2, n)), np.full((1, n), 3), np.zeros((1, n), dtype=int)]).astype(np.uint8)
    return np.vstack([sparse_strings(n, count, rng), full])


def _check_state(tensors, n, rng):
    S = _strings_for(n, rng)
    v, norm = ref_pauli_strings(tensors, S)
    vd, nd = pauli_strings_from_dense(dense(Q.MPS(tensors)), n, S)
    err = np.abs(v - vd).max()
    assert err < 1e-13, err
    assert abs(norm - nd) < 1e-13 * nd
    assert v[-1] == 1.0
    return S, v, norm


# ---- the reference against dense state vectors -----------------------------------------------------------------------
def test_reference_matches_dense_random_profiles_and_unnormalised():
    rng = np.random.default_rng(7)
    for prof in ([1, 2, 4, 8, 13, 9, 5, 3, 2, 1], [1, 2, 3, 6, 11, 7, 4, 2, 1], [1, 2, 1], [1, 1]):
        n = len(prof) - 1
        m = Q.random_mps(n, prof, rng)
        S, v, norm = _check_state(m.tensors, n, rng)
        scaled = [t * (3.7 if k == min(1, n - 1) else 1.0) for k, t in enumerate(m.tensors)]
        vs, ns = ref_pauli_strings(scaled, S)
        assert np.abs(vs - v).max() < 1e-13
        assert abs(ns - 3.7**2 * norm) < 1e-12 * ns


def test_reference_matches_dense_kernel_state_ansatz():
    rng = np.random.default_rng(3)
    ans = Q.KernelStateAnsatz(12, 2, 1.0, Q.entanglement_graph(12, 2))
    for x in R.synthetic_features(3, 12, 23):
        _check_state(Q.simulate(ans.circuit_for_data(x), 1 - 1e-16).tensors, 12, rng)


# ---- against the merged references -----------------------------------------------------------------------------------
def test_weight_one_strings_are_the_bloch_vectors_and_pair_strings_the_correlators():
    rng = np.random.default_rng(11)
    for prof in ([1, 2, 4, 8, 13, 9, 5, 3, 2, 1], [1, 2, 3, 6, 11, 7, 4, 2, 1], [1, 2, 1]):
        n = len(prof) - 1
        m = Q.random_mps(n, prof, rng)
        F, norm = ref_local_paulis(m.tensors)
        v, nv = ref_pauli_strings(m.tensors, weight_one_strings(n))
        assert np.abs(v.reshape(n, 3) - F).max() < 1e-13 and abs(nv - norm) < 1e-13 * norm
        D = min(3, n - 1)
        T, _ = ref_pair_paulis_dist(m.tensors, D)
        v2, _ = ref_pauli_strings(m.tensors, pair_strings(n, D))
        assert np.abs(v2.reshape(T.shape) - T).max() < 1e-13


# ---- analytic cases ---------------------------------------------------------------------------------------------------
def test_analytic_hadamard_xxphase_and_product_states():
    h = Q.simulate(Q.BoundCircuit.from_gates(1, [("H", [0], [])]), 1 - 1e-16)
    v, _ = ref_pauli_strings(h.tensors, engine.pauli_strings(1, ["X", "Y", "Z", "I"]))
    assert np.abs(v - [1.0, 0.0, 0.0, 1.0]).max() < 1e-13 and v[3] == 1.0
    for alpha in (0.3, -0.45, 0.5):
        m = Q.simulate(Q.BoundCircuit.from_gates(2, [("XXPhase", [0, 1], [alpha])]), 1 - 1e-16)
        v, _ = ref_pauli_strings(m.tensors, engine.pauli_strings(2, ["XY", "YX", "ZZ", "XX"]))
        s = math.sin(math.pi * alpha)
        assert np.abs(v - [-s, -s, 1.0, 0.0]).max() < 1e-13
    # a product state: the value of a string is the product of the Bloch components of its qubits
    n, a = 6, 0.37
    gates = [("Ry", [0], [a]), ("Rx", [1], [a]), ("H", [2], []), ("Ry", [4], [2 * a]), ("Rx", [5], [-a]), ("Ry", [3], [0.2]), ("Rx", [3], [0.6])]
    m = Q.simulate(Q.BoundCircuit.from_gates(n, gates), 1 - 1e-16)
    assert m.max_bond() == 1
    F, _ = ref_local_paulis(m.tensors)
    rng = np.random.default_rng(2)
    S = _strings_for(n, rng)
    v, _ = ref_pauli_strings(m.tensors, S)
    want = np.array([np.prod([F[k, c[k] - 1] for k in np.flatnonzero(c)]) for c in S])
    assert np.abs(v - want).max() < 1e-13


def test_parity_of_the_ansatz_without_hadamards_is_one():
    """Every gate of KernelStateAnsatz commutes with Z^(x)n (Rz and XXPhase), and |0..0> has parity +1."""
    n = 10
    ans = Q.KernelStateAnsatz(n, 2, 1.0, Q.entanglement_graph(n, 2), hadamard_init=False)
    for x in R.synthetic_features(4, n, 4)[:2]:
        m = Q.simulate(ans.circuit_for_data(x), 1 - 1e-16)
        assert m.max_bond() >= 8
        v, _ = ref_pauli_strings(m.tensors, engine.pauli_strings(n, ["Z" * n, "I" * n]))
        assert abs(v[0] - 1.0) < 1e-13 and v[1] == 1.0


# ---- the public surface without a device ------------------------------------------------------------------------------
def test_pauli_strings_spec_forms():
    S = engine.pauli_strings(6, ["IZXXZI", ("ZXZ", (3, 4, 5)), ("Y", [0]), [0, 1, 2, 3, 0, 0], np.array([3, 0, 0, 0, 0, 3], dtype=np.int64), ("", ())])
    assert S.dtype == np.uint8 and S.shape == (6, 6) and S.flags.c_contiguous
    assert S.tolist() == [[0, 3, 1, 1, 3, 0], [0, 0, 0, 3, 1, 3], [2, 0, 0, 0, 0, 0], [0, 1, 2, 3, 0, 0], [3, 0, 0, 0, 0, 3], [0] * 6]
    # qubits of a pair spec come in any order; an integer table passes through
    assert engine.pauli_strings(4, [("XZ", (3, 1))]).tolist() == [[0, 3, 0, 1]]
    tab = weight_one_strings(5)
    assert np.array_equal(engine.pauli_strings(5, tab), tab)
    assert np.array_equal(engine.pauli_strings(5, engine.pauli_strings(5, ["XXXXX", "IIIIZ"])), [[1] * 5, [0, 0, 0, 0, 3]])


@pytest.mark.parametrize(
    "spec",
    ["IZX", "IZXXZIZ", "IZAXZI", "izxxzi", ("ZX", (3,)), ("ZX", (3, 3)), ("ZX", (3, 6)), ("ZX", (-1, 2)), ("ZQ", (1, 2)), ("Z", 3),
     [0, 1, 2], [0, 1, 2, 3, 4, 0], [0, 1, -1, 3, 0, 0], [0.0, 1.0, 2.0, 3.0, 0.0, 0.0], None, 7, ("Z", (1,), 2), [[0] * 6]],
)
def test_pauli_strings_rejects_a_bad_spec_and_names_it(spec):
    with pytest.raises(ValueError) as e:
        engine.pauli_strings(6, ["IZXXZI", spec])
    assert repr(spec) in str(e.value)


def test_pauli_strings_rejects_an_empty_list_a_bare_spec_and_no_sites():
    with pytest.raises(ValueError, match="empty"):
        engine.pauli_strings(4, [])
    for bare in ("IZXI", ("ZX", (1, 2))):
        with pytest.raises(ValueError, match="list of specs"):
            engine.pauli_strings(4, bare)
    with pytest.raises(ValueError, match="n_sites"):
        engine.pauli_strings(0, ["I"])


class _FakeLib:
    """Stands in for the library: records the arguments of the Gram call and does nothing."""

    def __init__(self):
        self.calls = []

    def qk_feature_gram_host(self, h, m, nx, fx, ny, fy, g, out, ld):
        self.calls.append((m, nx, ny, g, ld))
        return 0


def test_feature_gram_checks_need_no_device(monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(engine, "lib", lambda: fake)
    ctx = engine.Context.__new__(engine.Context)  # the checks come before the handle is touched
    ctx._h = None
    assert engine.Context.feature_gram(ctx, np.zeros((3, 7))).shape == (3, 3)
    assert fake.calls[-1] == (7, 3, 3, 1.0 / 7, 3)  # the default bandwidth 1 / n_features
    assert engine.Context.feature_gram(ctx, np.zeros((3, 7)), np.zeros((2, 7)), gamma=0.3).shape == (2, 3)
    assert fake.calls[-1] == (7, 3, 2, 0.3, 3)
    for bad in (np.zeros((3, 0)), np.zeros(3), np.zeros((3, 2, 2))):
        with pytest.raises(ValueError, match="features"):
            engine.Context.feature_gram(ctx, bad)
    with pytest.raises(ValueError, match="do not match"):
        engine.Context.feature_gram(ctx, np.zeros((3, 7)), np.zeros((2, 6)))
    for g in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="bandwidth"):
            engine.Context.feature_gram(ctx, np.zeros((3, 7)), gamma=g)


@pytest.mark.parametrize(
    "kwargs,match",
    [
        ({"observables": []}, "empty"),
        ({"observables": ["ZZZ"]}, "ZZZ"),
        ({"observables": ["ZZZZ", ("X", (4,))]}, "bad Pauli string"),
        ({"observables": "ZZZZ"}, "list of specs"),
        ({"observables": ["ZZZZ"], "rdm": 2}, "rdm"),
        ({"observables": ["ZZZZ"], "rdm": 2, "pair_distance": 2}, "pair_distance"),
        ({"observables": ["ZZZZ"], "pair_distance": 2}, "pair_distance"),
        ({"observables": ["ZZZZ"], "pqk_gamma": 0.0}, "bandwidth"),
    ],
)
def test_build_projected_kernel_matrix_observables_argument_errors(monkeypatch, kwargs, match):
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend import kernel_state_ansatz as K

    def no_device(*a, **k):
        raise AssertionError("device work before the argument checks")

    monkeypatch.setattr(engine, "device_count", no_device)
    monkeypatch.setattr(engine, "default_context", no_device)
    ans = Q.KernelStateAnsatz(4, 1, 1.0, Q.entanglement_graph(4, 1))
    with pytest.raises(ValueError, match=match):
        K.build_projected_kernel_matrix(SingleComm(), ans, np.zeros((3, 4)), truncation_error=1e-16, **kwargs)


def test_library_exports_pauli_string_entry_points(built):
    L = engine.lib()
    for name in ("qk_pauli_strings_host", "qk_feature_gram_host"):
        assert name in engine.EXPORTED_SYMBOLS
        assert hasattr(L, name)
