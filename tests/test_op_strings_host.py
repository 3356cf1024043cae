"""Strings of single-site operators and outcome marginals on the host (no GPU): ``MPS.operator_expectation`` and ``MPS.marginal``
(the numpy mirrors of qk_operator_strings_host) against dense state vectors on 6-10 qubits, on canonical and on general-gauge
states; the identities the device tests rely on (Pauli table = Pauli strings, full-support projectors = |amplitude|^2, the
outcomes of a subset sum to 1, a window's Z marginals = the diagonal of its RDM, O^dagger = the complex conjugate);
``engine.LOCAL_OPS``, ``engine.operator_strings``, ``engine.marginal_strings`` and their rejections; the argument checks of
``build_outcome_marginals`` (raised before any device work) and the library's export."""
import itertools

import numpy as np
import pytest

import qml_cutensornet_amd as Q
from helpers import scrambled
from oracle import restatement as R
from qml_cutensornet_amd import engine
from test_pauli_strings_host import ref_pauli_strings, sparse_strings
from test_projected_host import dense


# ---- dense references ------------------------------------------------------------------------------------------------
def operator_strings_from_dense(psi, n, table, codes):
    """<psi| O_c[0] (x) ... |psi> / <psi|psi> from a dense state (qubit 0 = most significant axis), complex."""
    psi = np.asarray(psi).reshape((2,) * n)
    norm = float(np.vdot(psi, psi).real)
    vals = np.ones(len(codes), dtype=np.complex128)
    for m, c in enumerate(np.asarray(codes)):
        phi = psi
        for k in np.flatnonzero(c):
            phi = np.moveaxis(np.tensordot(table[c[k] - 1], phi, axes=(1, k)), 0, k)
        vals[m] = np.vdot(psi, phi) / norm
    return vals


def random_table(rng, n_ops=5):
    """Distinct random complex operators, every entry of magnitude < 1 (real and imaginary parts in [-0.7, 0.7])."""
    return (rng.uniform(-0.7, 0.7, size=(n_ops, 2, 2)) + 1j * rng.uniform(-0.7, 0.7, size=(n_ops, 2, 2))).astype(np.complex128)


def case_codes(n, rng, n_ops, count=24):
    """Random codes on sparse supports, then supports that start at site 0, end at site n - 1, a single site, an identity gap, the
    whole chain, the all-identity row and a duplicate of the first row."""
    S = sparse_strings(n, count, rng)
    S[S != 0] = rng.integers(1, n_ops + 1, size=int((S != 0).sum()))
    extra = np.zeros((7, n), dtype=np.uint8)
    extra[0, 0] = 1
    extra[1, n - 1] = n_ops
    extra[2, n // 2] = 2
    extra[3, 0], extra[3, min(2, n - 1)] = 3, 1
    extra[4, max(0, n - 4)], extra[4, n - 1] = 2, 3
    extra[5] = rng.integers(1, n_ops + 1, size=n)
    extra[6, 0], extra[6, n - 1] = n_ops, 1
    return np.ascontiguousarray(np.vstack([S, extra, np.zeros((1, n), dtype=np.uint8), S[:1]]))


def _states():
    """Canonical (right-orthonormal, and one scaled) and general-gauge states on 6-10 qubits, and a built ansatz state."""
    rng = np.random.default_rng(21)
    out = []
    for prof in ([1, 2, 4, 8, 13, 9, 5, 3, 2, 1], [1, 2, 3, 6, 4, 2, 1], [1, 2, 4, 7, 11, 16, 9, 5, 3, 2, 1]):
        m = Q.random_mps(len(prof) - 1, prof, rng)
        out += [m, scrambled(m, rng, scale=3.7), scrambled(m, rng, grow=2)]
    ans = Q.KernelStateAnsatz(8, 2, 1.0, Q.entanglement_graph(8, 2))
    out.append(Q.simulate(ans.circuit_for_data(R.synthetic_features(3, 8, 5)[0]), 1 - 1e-16))
    return out


# ---- the mirrors against dense state vectors --------------------------------------------------------------------------
def test_operator_expectation_matches_dense():
    rng = np.random.default_rng(5)
    for m in _states():
        n = len(m)
        assert 6 <= n <= 10
        table = random_table(rng)
        codes = case_codes(n, rng, len(table))
        v = m.operator_expectation(table, codes)
        ref = operator_strings_from_dense(dense(m), n, table, codes)
        assert v.shape == (len(codes),) and v.dtype == np.complex128
        assert np.abs(v - ref).max() < 1e-13
        assert v[-2] == 1.0 + 0.0j and v[-1] == v[0]  # all identity: exactly 1; the duplicate
        assert abs(v).max() > 1e-3 and np.abs(v.imag).max() > 1e-4  # the comparison is not between zeros
        one = m.operator_expectation(table, codes[3])
        assert np.shape(one) == () and one == v[3]


def test_marginal_matches_dense_and_sums_to_one():
    rng = np.random.default_rng(6)
    for m in _states():
        n = len(m)
        sub, basis = (0, 2, 3, n - 1), (1, 3, 2, 1)  # a non-contiguous subset in mixed bases
        bases = np.zeros(n, dtype=np.uint8)
        bases[list(sub)] = basis
        bits = np.zeros((16, n), dtype=np.uint8)
        bits[:, list(sub)] = list(itertools.product((0, 1), repeat=4))
        bits[:, 1] = rng.integers(0, 2, size=16)  # not measured: ignored
        p = m.marginal(bits, bases)
        table, codes = engine.marginal_strings(bits, bases, n)
        ref = operator_strings_from_dense(dense(m), n, table, codes)
        assert p.dtype == np.float64 and np.abs(p - ref.real).max() < 1e-13 and np.abs(ref.imag).max() < 1e-13
        assert abs(p.sum() - 1.0) < 1e-12 and p.min() > -1e-13
        # per-string bases; a row with no measured qubit is exactly 1.0
        B = np.vstack([bases, np.zeros(n, dtype=np.uint8), np.full(n, 3)])
        q = m.marginal(bits[:3], B)
        assert q[0] == p[0] and q[1] == 1.0


def test_full_support_projectors_are_squared_amplitudes_and_window_marginals_the_rdm_diagonal():
    rng = np.random.default_rng(8)
    for m in _states()[:6]:
        n = len(m)
        bases = engine.random_bases(5, n, 3)
        bits = rng.integers(0, 2, size=(5, n)).astype(np.uint8)
        amp = m.amplitude(bits, bases)
        norm = float(np.vdot(dense(m), dense(m)).real)
        p = m.marginal(bits, bases)
        assert np.abs(p - np.abs(amp) ** 2 / norm).max() < 1e-13 * max(1.0, p.max())
        a, w = 2, 3
        zb = np.zeros(n, dtype=np.uint8)
        zb[a : a + w] = 3
        zbits = np.zeros((8, n), dtype=np.uint8)
        zbits[:, a : a + w] = list(itertools.product((0, 1), repeat=w))
        assert np.abs(m.marginal(zbits, zb) - np.diag(m.window_rdm(a, w)).real).max() < 1e-13


def test_pauli_table_and_adjoint_and_linearity():
    rng = np.random.default_rng(9)
    m = _states()[1]
    n = len(m)
    S = sparse_strings(n, 20, rng)
    pauli = np.stack([engine.LOCAL_OPS[c] for c in "XYZ"])
    v = m.operator_expectation(pauli, S)
    ref, _ = ref_pauli_strings(m.tensors, S)
    assert np.abs(v.real - ref).max() < 1e-13 and np.abs(v.imag).max() < 1e-13
    table = random_table(rng)
    codes = case_codes(n, rng, len(table))
    va = m.operator_expectation(table, codes)
    vd = m.operator_expectation(table.conj().transpose(0, 2, 1), codes)
    assert np.abs(vd - va.conj()).max() < 1e-13
    # a confusion-matrix mix of the two projectors of a site is the same mix of the two marginals
    eps0, eps1 = 0.03, 0.08
    M0 = (1 - eps0) * engine.LOCAL_OPS["0"] + eps1 * engine.LOCAL_OPS["1"]  # read 0: true 0 kept, true 1 flipped
    t2 = np.stack([engine.LOCAL_OPS["0"], engine.LOCAL_OPS["1"], engine.LOCAL_OPS["+"], M0])
    rows = np.zeros((3, n), dtype=np.uint8)
    rows[:, 1] = 3
    rows[:, 4] = (4, 1, 2)
    mix = m.operator_expectation(t2, rows)
    assert abs(mix[0] - ((1 - eps0) * mix[1] + eps1 * mix[2])) < 1e-13


# ---- engine.LOCAL_OPS, operator_strings, marginal_strings ---------------------------------------------------------------
def test_local_ops():
    ops = engine.LOCAL_OPS
    assert sorted(ops) == sorted(["I", "X", "Y", "Z", "0", "1", "+", "-", "R", "L", "01", "10"])
    for name, m in ops.items():
        assert m.shape == (2, 2) and m.dtype == np.complex128, name
    for plus, minus, pauli in (("0", "1", "Z"), ("+", "-", "X"), ("R", "L", "Y")):
        assert np.array_equal(ops[plus] + ops[minus], ops["I"])
        assert np.array_equal(ops[plus] - ops[minus], ops[pauli])  # eigenvalue +1 is outcome bit 0
        assert np.array_equal(ops[plus] @ ops[plus], ops[plus])
    assert np.array_equal(ops["01"], [[0, 1], [0, 0]]) and np.array_equal(ops["10"], ops["01"].T)
    # the sampler's convention: bit 0 in the Y basis is (<0| - i <1|) / sqrt2, so its projector is "R"
    r = np.array([1, 1j]) / np.sqrt(2)
    assert np.abs(np.outer(r, r.conj()) - ops["R"]).max() < 1e-15


def test_operator_strings_spec_forms():
    table, codes = engine.operator_strings(6, [("0+R", (1, 4, 5)), (("01", "10"), (2, 0)), ("I0", (3, 1)), ("", ())])
    assert table.dtype == np.complex128 and table.shape == (5, 2, 2) and codes.dtype == np.uint8 and codes.flags.c_contiguous
    assert codes.tolist() == [[0, 1, 0, 0, 2, 3], [5, 0, 4, 0, 0, 0], [0, 1, 0, 0, 0, 0], [0] * 6]
    for c, name in enumerate(["0", "+", "R", "01", "10"]):
        assert np.array_equal(table[c], engine.LOCAL_OPS[name])
    # a user dict wins over LOCAL_OPS; names of any length go in a sequence
    mine = {"Zd": [[0.9, 0], [0, -0.8]], "X": [[0, 0.5], [0.5, 0]]}
    table, codes = engine.operator_strings(3, [(("Zd", "X"), (0, 2)), ("X1", (0, 1))], ops=mine)
    assert codes.tolist() == [[1, 0, 2], [2, 3, 0]]
    assert np.array_equal(table[0], np.array(mine["Zd"])) and np.array_equal(table[1], np.array(mine["X"])) and np.array_equal(table[2], engine.LOCAL_OPS["1"])
    # rows of codes into a user table: the table passes through
    user = np.arange(24, dtype=np.float64).reshape(3, 2, 2, 2)
    user = (user[..., 0] + 1j * user[..., 1]) / 32
    table, codes = engine.operator_strings(4, np.array([[0, 3, 1, 0], [2, 0, 0, 0]]), ops=user)
    assert np.array_equal(table, user) and codes.tolist() == [[0, 3, 1, 0], [2, 0, 0, 0]]
    table, codes = engine.operator_strings(4, [[0, 3, 1, 0]], ops=user)
    assert codes.tolist() == [[0, 3, 1, 0]]
    # only identities: the table is not empty, the row is all zero
    table, codes = engine.operator_strings(2, [("II", (0, 1))])
    assert table.shape == (1, 2, 2) and codes.tolist() == [[0, 0]]


@pytest.mark.parametrize(
    "spec",
    [("0+", (3,)), ("0+", (3, 3)), ("0+", (3, 6)), ("0+", (-1, 2)), ("0Q", (1, 2)), (("0", "nope"), (1, 2)), ("0", 3), [0, 1, 2, 0, 0, 0], None, 7, "0+R1-L",
     ("0", (1,), 2)],
)
def test_operator_strings_rejects_a_bad_spec_and_names_it(spec):
    with pytest.raises(ValueError) as e:
        engine.operator_strings(6, [("0+R", (1, 4, 5)), spec])
    assert repr(spec) in str(e.value)


@pytest.mark.parametrize("spec", [[0, 1, 2], [0, 1, 4, 0, 0, 0], [0, 1, -1, 3, 0, 0], [0.0, 1.0, 2.0, 3.0, 0.0, 0.0], ("0+", (1, 2)), [[0] * 6]])
def test_operator_strings_rejects_a_bad_row_of_codes_and_names_it(spec):
    user = np.stack([engine.LOCAL_OPS[c] for c in "XYZ"])
    with pytest.raises(ValueError) as e:
        engine.operator_strings(6, [[0, 3, 1, 0, 0, 2], spec], ops=user)
    assert repr(spec) in str(e.value)


def test_operator_strings_rejects_bad_tables_lists_and_sizes():
    with pytest.raises(ValueError, match="empty"):
        engine.operator_strings(4, [])
    with pytest.raises(ValueError, match="list of specs"):
        engine.operator_strings(4, ("0+", (1, 2)))
    with pytest.raises(ValueError, match="n_sites"):
        engine.operator_strings(0, [("0", (0,))])
    for bad in (np.zeros((0, 2, 2)), np.zeros((256, 2, 2)), np.zeros((3, 2, 3)), np.zeros((2, 2))):
        with pytest.raises(ValueError, match="n_ops"):
            engine.operator_strings(4, [[0, 0, 0, 0]], ops=bad)
    nan = np.zeros((3, 2, 2), dtype=np.complex128)
    nan[1, 1, 0] = complex(0.0, float("inf"))
    with pytest.raises(ValueError, match=r"operator 2 .*\[1\]\[0\]"):
        engine.operator_strings(4, [[0, 0, 0, 0]], ops=nan)
    for name, mat in (("A", np.zeros((2, 3))), ("B", [[float("nan"), 0], [0, 1]]), ("", np.eye(2)), (3, np.eye(2))):
        with pytest.raises(ValueError, match=repr(name)):
            engine.operator_strings(4, [("0", (1,))], ops={name: mat})
    # more than 255 distinct operators
    many = {f"o{i}": np.eye(2) * (i + 1) / 300 for i in range(256)}
    with pytest.raises(ValueError, match="255"):
        engine.operator_strings(256, [(tuple(many), tuple(range(256)))], ops=many)


def test_marginal_strings_and_rejections():
    bits = np.array([[0, 1, 1, 0], [1, 1, 0, 0]])
    table, codes = engine.marginal_strings(bits, [3, 0, 1, 2], 4)
    assert [np.array_equal(table[i], engine.LOCAL_OPS[c]) for i, c in enumerate("+-RL01")] == [True] * 6
    assert codes.dtype == np.uint8 and codes.tolist() == [[5, 0, 2, 3], [6, 0, 1, 3]]
    _, codes = engine.marginal_strings(bits, [[3, 0, 1, 2], [0, 0, 0, 0]], 4)
    assert codes.tolist() == [[5, 0, 2, 3], [0, 0, 0, 0]]
    _, codes = engine.marginal_strings(np.array([[0, 7, 1, 0]]), [3, 0, 1, 2], 4)  # the bit of an unmeasured qubit is ignored
    assert codes.tolist() == [[5, 0, 2, 3]]
    for bad_bits in (np.zeros(4, dtype=int), np.zeros((2, 3), dtype=int), np.zeros((2, 4)), np.zeros((0, 4), dtype=int)):
        with pytest.raises(ValueError, match="bits"):
            engine.marginal_strings(bad_bits, [3, 0, 1, 2], 4)
    with pytest.raises(ValueError, match="bits"):
        engine.marginal_strings(np.array([[0, 1, 2, 0]]), [3, 0, 1, 2], 4)
    for bad_bases in ([3, 0, 1], [[3, 0, 1, 2]] * 3, [3.0, 0.0, 1.0, 2.0], [3, 0, 4, 2], [3, 0, -1, 2]):
        with pytest.raises(ValueError, match="bases"):
            engine.marginal_strings(bits, bad_bases, 4)


def test_mirror_rejections():
    m = Q.random_mps(4, [1, 2, 4, 2, 1], np.random.default_rng(0))
    pauli = np.stack([engine.LOCAL_OPS[c] for c in "XYZ"])
    for codes in ([0, 1, 2], [[0, 1, 2, 4]], [0.0, 1.0, 0.0, 0.0], np.zeros((0, 4), dtype=int)):
        with pytest.raises(ValueError, match="codes"):
            m.operator_expectation(pauli, codes)
    with pytest.raises(ValueError, match="n_ops"):
        m.operator_expectation(np.zeros((2, 2)), [0, 1, 0, 0])
    zero = Q.MPS([t * 0 for t in m.tensors])
    with pytest.raises(ValueError, match="norm 0"):
        zero.operator_expectation(pauli, [0, 1, 0, 0])


@pytest.mark.parametrize(
    "kwargs,match",
    [
        ({"bits": np.zeros((2, 3), dtype=int), "bases": [3, 3, 0, 0]}, "bits"),
        ({"bits": np.zeros((2, 4), dtype=int), "bases": [3, 3, 0]}, "bases"),
        ({"bits": np.zeros((2, 4), dtype=int), "bases": [3, 4, 0, 0]}, "bases"),
        ({"bits": np.zeros((2, 4), dtype=int), "bases": [3, 3, 0, 0], "truncation_error": None}, "truncation error"),
    ],
)
def test_build_outcome_marginals_argument_errors(monkeypatch, kwargs, match):
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend import kernel_state_ansatz as K

    def no_device(*a, **k):
        raise AssertionError("device work before the argument checks")

    monkeypatch.setattr(engine, "device_count", no_device)
    monkeypatch.setattr(engine, "default_context", no_device)
    ans = Q.KernelStateAnsatz(4, 1, 1.0, Q.entanglement_graph(4, 1))
    kwargs = {"truncation_error": 1e-16, **kwargs}
    with pytest.raises(ValueError, match=match):
        K.build_outcome_marginals(SingleComm(), ans, np.zeros((3, 4)), **kwargs)


def test_library_exports_the_entry_point(built):
    assert "qk_operator_strings_host" in engine.EXPORTED_SYMBOLS
    assert hasattr(engine.lib(), "qk_operator_strings_host")
