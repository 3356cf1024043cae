"""MPO observables on the host (no GPU): ``engine.Mpo`` and its constructors against explicit Kronecker sums on at most 8 qubits
(``mpo_from_terms`` with one-site terms, overlapping hulls, duplicates and ladder operators; ``mpo_exponential``; ``mpo_product``),
``+``, ``@``, ``scale`` and ``dagger`` against dense matrices, the states of the finite-state machine at every cut,
``MPS.mpo_expectation`` (the numpy mirror of qk_mpo_expectations_host) against ``psi^dagger H psi`` of dense vectors on canonical
and general-gauge states of 8 to 10 sites, every rejection of the Python layer, the library's export, and the operator bounds
that scale the tolerances of tests/test_gpu_mpo.py: the random dense MPOs have every matricised tensor at spectral norm 1 (so
||H|| <= 1) and a term-built MPO has S = sum_t |c_t| prod ||O||_2 >= ||H||."""
import functools
import itertools

import numpy as np
import pytest

import qml_cutensornet_amd as Q
from helpers import scrambled
from qml_cutensornet_amd import engine
from test_projected_host import dense

LADDER = {"Sp": [[0, 1], [0, 0]], "Sm": [[0, 0], [1, 0]], "G": [[0.3, 0.2 - 0.5j], [0.1j, -0.4]]}  # not Hermitian


# ---- term lists and MPOs shared with tests/test_gpu_mpo.py ---------------------------------------------------------------
def heisenberg_terms(n, sites=None, J=(1.0, 0.8, -0.6), h=0.5):
    """A Heisenberg chain with a field on ``sites`` (default: every qubit): J_x XX + J_y YY + J_z ZZ on neighbours, h Z on each."""
    sites = list(range(n)) if sites is None else list(sites)
    terms = [(j, p + p, (a, b)) for a, b in zip(sites, sites[1:]) for j, p in zip(J, "XYZ")]
    return terms + [(h, "Z", (a,)) for a in sites]


def exponential_terms(n, a, b, J, lam):
    return [(J * lam ** (j - i - 1), (a, b), (i, j)) for i in range(n) for j in range(i + 1, n)]


def hamming_terms(qubits, weight):
    """The projector onto the bit strings of Hamming weight ``weight`` on ``qubits``: one product of projectors per string."""
    return [(1.0, "".join(str(b) for b in bits), tuple(qubits)) for bits in itertools.product((0, 1), repeat=len(qubits)) if sum(bits) == weight]


def term_bound(terms, ops=None):
    """S = sum_t |c_t| prod_k ||O_k||_2: an upper bound of ||H||."""
    named = {k: np.asarray(v, dtype=complex) for k, v in (ops or {}).items()}
    norm = lambda name: float(np.linalg.norm(named[name] if name in named else engine.LOCAL_OPS[name], ord=2))
    return float(sum(abs(c) * np.prod([norm(x) for x in names]) for c, names, _ in terms))


def random_dense_mpo(rng, bonds):
    """A random complex MPO with the given bonds, every tensor matricised as (u, s') x (v, s) and scaled to spectral norm 1."""
    ts = []
    for wl, wr in zip(bonds, bonds[1:]):
        t = rng.uniform(-1, 1, size=(wl, wr, 2, 2)) + 1j * rng.uniform(-1, 1, size=(wl, wr, 2, 2))
        ts.append(t / np.linalg.norm(t.transpose(0, 2, 1, 3).reshape(2 * wl, 2 * wr), ord=2))
    return engine.Mpo(ts)


def matricised_norms(mpo):
    return [float(np.linalg.norm(t.transpose(0, 2, 1, 3).reshape(2 * t.shape[0], 2 * t.shape[1]), ord=2)) for t in mpo.tensors]


def kron_sum(n, terms, ops=None):
    """sum_t c_t (x)_k O_k as a 2^n x 2^n matrix, qubit 0 the most significant bit."""
    named = {k: np.asarray(v, dtype=complex) for k, v in (ops or {}).items()}
    H = np.zeros((2**n, 2**n), dtype=complex)
    for c, names, qubits in terms:
        site = {int(q): (named[x] if x in named else engine.LOCAL_OPS[x]) for x, q in zip(names, qubits)}
        H += c * functools.reduce(np.kron, [site.get(k, np.eye(2)) for k in range(n)])
    return H


TERM_CASES = {  # name: (n, terms, ops)
    "heisenberg": (7, heisenberg_terms(7), None),
    "one-site only": (5, [(0.3, "X", (1,)), (-1.2j, "Z", (1,)), (0.7, "Y", (4,)), (2.0, "0", (0,))], None),
    "overlapping hulls": (8, [(1.0, "XZ", (0, 5)), (0.5, "YY", (2, 3)), (-0.25, "ZXZ", (1, 4, 7)), (2.0, "X", (3,)), (1.5j, "Z1", (3, 6)), (0.1, "+-", (6, 7))], None),
    "duplicates": (6, [(1.0, "XX", (1, 4)), (1.0, "XX", (1, 4)), (-0.5, "XX", (1, 4)), (0.25, "Z", (2,)), (0.25, "Z", (2,))], None),
    "ladder": (6, [(1.0, ("Sp", "Sm"), (0, 1)), (0.7 - 0.2j, ("Sm", "G", "Sp"), (1, 3, 5)), (1.0, ("G",), (2,)), (0.4, ("Sp", "Z"), (4, 5))], LADDER),
    "hamming": (8, hamming_terms((1, 2, 4, 6, 7), 3), None),
    "one qubit": (1, [(0.5, "X", (0,)), (2.0, "Z", (0,))], None),
    "unordered qubits": (5, [(1.0, "XZ", (4, 1)), (1.0, "Y0", (3, 0))], None),
}


@pytest.mark.parametrize("name", sorted(TERM_CASES))
def test_mpo_from_terms_against_the_kronecker_sum(name):
    n, terms, ops = TERM_CASES[name]
    H = engine.mpo_from_terms(n, terms, ops)
    assert H.n_sites == n and H.bonds[0] == H.bonds[-1] == 1 and H.bonds.dtype == np.int32
    ref = kron_sum(n, terms, ops)
    assert np.abs(H.to_dense() - ref).max() < 1e-14 * max(1.0, term_bound(terms, ops))
    assert np.linalg.norm(ref, ord=2) <= term_bound(terms, ops) * (1 + 1e-12)


def test_the_states_of_the_machine_at_every_cut():
    n = 8
    terms = [(1.0, "XZ", (0, 5)), (0.5, "YY", (2, 3)), (-0.25, "ZXZ", (1, 4, 7)), (2.0, "X", (3,)), (1.0, "ZZ", (6, 7))]
    first, last = [0, 2, 1, 3, 6], [5, 3, 7, 3, 7]
    H = engine.mpo_from_terms(n, terms)
    for k in range(n + 1):
        want = int(any(f >= k for f in first)) + sum(f < k <= e for f, e in zip(first, last)) + int(any(e < k for e in last))
        assert H.bonds[k] == want, (k, H.bonds)
    # cut 3: start, terms 0, 1, 2 in term order, no done yet; site 3 carries the one-site term from start to done
    assert list(H.bonds[:5]) == [1, 2, 3, 4, 4]
    W3 = H.tensors[3]
    assert np.array_equal(W3[0, 0], np.eye(2)) and np.array_equal(W3[0, 3], 2.0 * engine.LOCAL_OPS["X"])  # start -> start, start -> done
    assert np.array_equal(W3[1, 1], np.eye(2))  # term 0 (qubits 0, 5): identity on a hull site outside its support
    assert np.array_equal(W3[2, 3], engine.LOCAL_OPS["Y"])  # term 1 ends here: into done
    assert np.array_equal(H.tensors[2][0, 2], 0.5 * engine.LOCAL_OPS["Y"])  # the coefficient sits on the first site
    # a support inside the chain: the sites outside hold the exact 1 x 1 identity
    inner = engine.mpo_from_terms(9, [(1.0, "ZZ", (a, a + 1)) for a in range(3, 6)])
    assert list(inner.bonds) == [1, 1, 1, 1, 2, 3, 2, 1, 1, 1]  # cut 6: the last term is open, nothing can start any more
    for k in (0, 1, 2, 7, 8):
        assert np.array_equal(inner.tensors[k], np.eye(2).reshape(1, 1, 2, 2))


@pytest.mark.parametrize("n", [2, 3, 4, 7])
def test_mpo_exponential_against_the_kronecker_sum(n):
    for a, b, J, lam in (("Z", "Z", 1.0, 0.7), ("X", "Y", -0.5 + 0.25j, 0.3), ("Sp", "Sm", 2.0, -0.9)):
        A, B = (LADDER.get(x, x) for x in (a, b))
        H = engine.mpo_exponential(n, A, B, J, lam)
        assert H.max_bond() == min(3, n - 1) and H.n_sites == n
        terms = exponential_terms(n, a, b, J, lam)
        assert np.abs(H.to_dense() - kron_sum(n, terms, LADDER)).max() < 1e-14 * term_bound(terms, LADDER)


def test_mpo_product_is_the_bond_one_string():
    n = 6
    P = engine.mpo_product(n, "X0R", (4, 1, 2))
    assert list(P.bonds) == [1] * (n + 1)
    assert np.abs(P.to_dense() - kron_sum(n, [(1.0, "X0R", (4, 1, 2))])).max() == 0.0
    for k in (0, 3, 5):
        assert np.array_equal(P.tensors[k], np.eye(2).reshape(1, 1, 2, 2))
    table = np.stack([np.asarray(LADDER["G"], dtype=complex), engine.LOCAL_OPS["01"]])
    T = engine.mpo_product(n, table, [0, 2, 0, 1, 1, 0])
    assert np.abs(T.to_dense() - kron_sum(n, [(1.0, ("01", "G", "G"), (1, 3, 4))], LADDER)).max() < 1e-15
    ident = engine.mpo_product(n, "", ())
    assert np.array_equal(ident.to_dense(), np.eye(2**n))


def test_sum_product_scale_and_dagger_against_dense():
    rng = np.random.default_rng(4)
    n = 5
    A, B = random_dense_mpo(rng, [1, 3, 5, 2, 4, 1]), random_dense_mpo(rng, [1, 2, 2, 3, 1, 1])
    a, b = A.to_dense(), B.to_dense()
    S, M = A + B, A @ B
    assert list(S.bonds) == [1, 5, 7, 5, 5, 1] and list(M.bonds) == [1, 6, 10, 6, 4, 1]
    assert np.abs(S.to_dense() - (a + b)).max() < 1e-14
    assert np.abs(M.to_dense() - a @ b).max() < 1e-14
    assert np.abs(A.dagger().to_dense() - a.conj().T).max() == 0.0
    assert np.abs(A.scale(2 - 1j).to_dense() - (2 - 1j) * a).max() < 1e-15
    assert np.array_equal(A.scale(2).to_dense(), 2 * a)  # a power of two: exact
    one = engine.Mpo([rng.standard_normal((1, 1, 2, 2))])
    assert np.abs((one + one).to_dense() - 2 * one.to_dense()).max() < 1e-15
    H = engine.mpo_from_terms(n, heisenberg_terms(n))
    assert np.abs((H @ H).to_dense() - H.to_dense() @ H.to_dense()).max() < 1e-12 and (H @ H).max_bond() == 25


def test_random_dense_mpos_are_bounded_by_one():
    rng = np.random.default_rng(6)
    for bonds in ([1, 3, 5, 2, 4, 1], [1, 2, 6, 3, 1, 2, 1]):
        H = random_dense_mpo(rng, bonds)
        assert np.allclose(matricised_norms(H), 1.0, rtol=0, atol=1e-14)
        assert np.linalg.norm(H.to_dense(), ord=2) <= 1.0 + 1e-12


def _states():
    rng = np.random.default_rng(31)
    out = []
    for prof in ([1, 2, 4, 8, 13, 8, 4, 2, 1], [1, 2, 4, 7, 11, 16, 9, 5, 3, 2, 1], [1, 2, 3, 6, 8, 6, 4, 3, 2, 1]):
        m = Q.random_mps(len(prof) - 1, prof, rng)
        out += [m, scrambled(m, rng, scale=3.7), scrambled(m, rng, grow=2)]
    return out


def test_mpo_expectation_against_dense_vectors():
    rng = np.random.default_rng(8)
    worst = 0.0
    for m in _states():
        n = len(m)
        assert 8 <= n <= 10
        psi = dense(m).reshape(-1)
        norm = float(np.vdot(psi, psi).real)
        terms = heisenberg_terms(n) + [(0.3 - 0.4j, ("Sp", "Sm"), (1, n - 2))]
        cases = [(engine.mpo_from_terms(n, terms, LADDER), term_bound(terms, LADDER)), (engine.mpo_exponential(n, "Z", "X", 1.0, 0.7), term_bound(exponential_terms(n, "Z", "X", 1.0, 0.7))),
                 (random_dense_mpo(rng, [1, 3, 5, 2] + [4] * (n - 4) + [1]), 1.0), (engine.mpo_from_terms(n, hamming_terms((0, 2, 3, 5, n - 1), 3)), 10.0)]
        for H, S in cases:
            v = m.mpo_expectation(H)
            ref = np.vdot(psi, H.to_dense() @ psi) / norm
            assert isinstance(v, complex)
            worst = max(worst, abs(v - ref) / S)
            assert abs(v - ref) < 1e-13 * S
        assert m.mpo_expectation(engine.mpo_product(n, "", ())) == 1.0 + 0.0j
        table = np.stack([np.asarray(LADDER["G"], dtype=complex), engine.LOCAL_OPS["Y"]])
        codes = np.zeros(n, dtype=np.uint8)
        codes[[1, 4, n - 1]] = (1, 2, 1)
        assert abs(m.mpo_expectation(engine.mpo_product(n, table, codes)) - m.operator_expectation(table, codes)) < 1e-14
    print(f"MPS.mpo_expectation against dense vectors: max |d| / S = {worst:.3e}")


def test_rejections_of_the_python_layer():
    eye = np.eye(2).reshape(1, 1, 2, 2)
    for bad, match in (([], "at least one site"), ([np.zeros((1, 2, 2))], "shape"), ([np.zeros((1, 2, 2, 2)), np.zeros((3, 1, 2, 2))], "cut 1"),
                       ([np.zeros((2, 1, 2, 2))], "bond 1"), ([np.zeros((1, 33, 2, 2)), np.zeros((33, 1, 2, 2))], "cut 1, above MPO_MAX_BOND = 32"),
                       ([eye, np.full((1, 1, 2, 2), np.nan)], r"tensor 1 has an entry \[0\]\[0\]\[0\]\[0\] that is not finite"), ([["x"]], "sequence of complex arrays")):
        with pytest.raises(ValueError, match=match):
            engine.Mpo(bad)
    A = engine.Mpo([eye, eye])
    with pytest.raises(ValueError, match="2 and 3 sites"):
        A + engine.Mpo([eye] * 3)
    with pytest.raises(ValueError, match="2 and 3 sites"):
        A @ engine.Mpo([eye] * 3)
    with pytest.raises(TypeError):
        A + 1
    with pytest.raises(ValueError, match="finite"):
        A.scale(float("inf"))
    with pytest.raises(ValueError, match="at most 12 sites"):
        engine.Mpo([eye] * 13).to_dense()
    # a cut above 32 states is named: 31 open terms, then start and done as well at cut 32
    many = [(1.0, "ZZ", (a, 40)) for a in range(31)] + [(1.0, "X", (31,)), (1.0, "X", (33,))]
    assert engine.mpo_from_terms(41, many[:-2] + many[-1:]).max_bond() == 32
    with pytest.raises(ValueError, match="33 states at cut 32, above MPO_MAX_BOND = 32"):
        engine.mpo_from_terms(41, many)
    for bad, match in (([], "empty"), ([(1.0, "X")], "term 0 is not a triple"), ([(1.0, "X", (0,)), ("a", "X", (0,))], "term 1 has a coefficient"),
                       ([(float("nan"), "X", (0,))], "not finite"), ([(1.0, "Q", (0,))], "Q"), ([(1.0, "XX", (0, 0))], "distinct"), ([(1.0, "I", (2,))], "term 0 acts on no qubit")):
        with pytest.raises(ValueError, match=match):
            engine.mpo_from_terms(4, bad)
    with pytest.raises(ValueError, match="n_sites >= 2"):
        engine.mpo_exponential(1, "Z", "Z", 1.0, 0.5)
    with pytest.raises(ValueError, match="LOCAL_OPS"):
        engine.mpo_exponential(4, "Q", "Z", 1.0, 0.5)
    with pytest.raises(ValueError, match="2 x 2"):
        engine.mpo_exponential(4, np.eye(3), "Z", 1.0, 0.5)
    with pytest.raises(ValueError, match="finite"):
        engine.mpo_exponential(4, "Z", "Z", float("nan"), 0.5)
    m = Q.random_mps(4, [1, 2, 4, 2, 1], np.random.default_rng(0))
    with pytest.raises(ValueError, match="2 sites, the state has 4"):
        m.mpo_expectation(A)
    with pytest.raises(ValueError, match="engine.Mpo"):
        m.mpo_expectation([eye] * 4)
    with pytest.raises(ValueError, match="norm 0"):
        Q.MPS([t * 0 for t in m.tensors]).mpo_expectation(engine.Mpo([eye] * 4))
    for bad, n_sites, match in ((A, 2, "single Mpo"), ([], 2, "empty"), ([A, 3], 2, "entry 1"), ([A], 4, "Mpo 0 has 2 sites, the states have 4")):
        with pytest.raises(ValueError, match=match):
            engine._mpo_list(bad, n_sites)


def test_driver_arguments_are_checked_before_any_device_work():
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_mpo_expectations, build_projected_kernel_matrix

    n = 4
    ans = Q.KernelStateAnsatz(n, 1, 1.0, Q.entanglement_graph(n, 1))
    X = np.zeros((2, n))
    H = engine.mpo_from_terms(n, heisenberg_terms(n))
    with pytest.raises(ValueError, match="truncation error"):
        build_mpo_expectations(SingleComm(), ans, X, [H])
    with pytest.raises(ValueError, match="Mpo 0 has 5 sites"):
        build_mpo_expectations(SingleComm(), ans, X, [engine.mpo_from_terms(5, heisenberg_terms(5))], truncation_error=1e-16)
    with pytest.raises(ValueError, match="mixes Mpo and Pauli strings"):
        build_projected_kernel_matrix(SingleComm(), ans, X, observables=[H, "XXII"], truncation_error=1e-16)
    with pytest.raises(ValueError, match="shots together with observables"):
        build_projected_kernel_matrix(SingleComm(), ans, X, observables=[H], shots=10, truncation_error=1e-16)
    with pytest.raises(ValueError, match="Mpo 1 has 5 sites"):
        build_projected_kernel_matrix(SingleComm(), ans, X, observables=[H, engine.mpo_from_terms(5, heisenberg_terms(5))], truncation_error=1e-16)


def test_the_library_exports_the_entry():
    assert hasattr(engine.lib(), "qk_mpo_expectations_host") and engine.MPO_MAX_BOND == 32
