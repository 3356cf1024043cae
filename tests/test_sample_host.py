"""Measurement shots on the host (no GPU): the Philox4x32-10 of ``engine.philox4x32`` against Random123's known answers, the numpy
mirror ``MPS.sample`` (perfect sampling along the chain, every shot and qubit in its own Pauli basis) against dense state vectors --
the probability it reports for a drawn string is the Born probability of that string in those bases --, its invariance under the
norm of the state, circuits whose outcomes are certain, and the estimators that turn shots into the Bloch vectors and Pauli
correlators the projected kernels take."""
import functools

import numpy as np
import pytest

import qml_cutensornet_amd as Q
from oracle import restatement as R
from qml_cutensornet_amd import engine

H2 = 0.70710678118654752440
# <outcome o| in basis code c, as a row over the physical index: X: <+|, <-|; Y: <+i|, <-i|; Z: <0|, <1|
OUTCOME_ROWS = {
    1: np.array([[H2, H2], [H2, -H2]], dtype=complex),
    2: np.array([[H2, -1j * H2], [H2, 1j * H2]], dtype=complex),
    3: np.array([[1, 0], [0, 1]], dtype=complex),
}


def ansatz_states(n, layers, count, seed, hadamard_init=True):
    """``count`` states of KernelStateAnsatz(n, layers, 1.0, entanglement_graph(n, 2)) at truncation error 1e-16, with their circuits.
    The features lie in [0, 0.5] or [1.5, 2]: away from 1 the XXPhase exponents gamma^2 (1 - f_a)(1 - f_b) are large and the bonds grow."""
    ans = Q.KernelStateAnsatz(n, layers, 1.0, Q.entanglement_graph(n, 2), hadamard_init=hadamard_init)
    rng = np.random.default_rng(seed)
    X = np.where(rng.random((count, n)) < 0.5, rng.uniform(0.0, 0.5, (count, n)), rng.uniform(1.5, 2.0, (count, n)))
    circs = [ans.circuit_for_data(x) for x in X]
    return [Q.simulate(c, 1 - 1e-16) for c in circs], circs


def dense_of_circuit(circ):
    """The state vector of a bound circuit as a (2,) * n array, qubit k = axis k."""
    psi = R.statevector(circ.n_qubits, [(name, tuple(qs), (p[0] if p else None)) for name, qs, p in circ.as_tuples()])
    return np.asarray(psi).reshape((2,) * circ.n_qubits)


def dense_of_mps(m):
    """The dense amplitudes of an MPS as a (2,) * n array, qubit k = axis k."""
    psi = np.ones((1, 1), dtype=complex)
    for t in m.tensors:
        psi = np.tensordot(psi, np.asarray(t, dtype=complex), axes=(psi.ndim - 1, 0))
    return psi.reshape((2,) * len(m.tensors))


def dense_probability(psi, bits, bases):
    """|<b| U_bases |psi>|^2 / <psi|psi> of every shot: bits and bases (shots, n), psi (2,) * n."""
    n = psi.ndim
    norm = float(np.vdot(psi, psi).real)
    out = np.zeros(len(bits))
    for s, (b, c) in enumerate(zip(bits, bases)):
        amp = psi
        for k in range(n):
            amp = np.tensordot(OUTCOME_ROWS[int(c[k])][int(b[k])], amp, axes=(0, 0))
        out[s] = abs(complex(amp)) ** 2 / norm
    return out


@functools.lru_cache(maxsize=None)
def nine_qubit_case():
    states, circs = ansatz_states(9, 2, 3, 21)
    return states, [dense_of_circuit(c) for c in circs]


def test_philox_known_answers():
    # Random123's known-answer vectors for philox4x32-10
    assert [int(x) for x in engine.philox4x32([0, 0, 0, 0], [0, 0])] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    ones = 0xFFFFFFFF
    assert [int(x) for x in engine.philox4x32([ones] * 4, [ones] * 2)] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    # vectorised: rows of a table are the single calls
    table = engine.philox4x32([[0, 0, 0, 0], [ones] * 4, [1, 2, 3, 4]], [[0, 0], [ones] * 2, [5, 6]])
    assert table.shape == (3, 4) and table.dtype == np.uint32
    assert np.array_equal(table[0], engine.philox4x32([0, 0, 0, 0], [0, 0])) and np.array_equal(table[2], engine.philox4x32([1, 2, 3, 4], [5, 6]))


def test_sample_uniform_and_random_bases():
    u = engine.sample_uniform(2**63 + 11, np.arange(7)[:, None, None], np.arange(50)[None, :, None], np.arange(13)[None, None, :])
    assert u.shape == (7, 50, 13) and u.dtype == np.float64
    assert np.all(u >= 0.0) and np.all(u < 1.0)
    assert 0.45 < u.mean() < 0.55 and len(np.unique(u)) == u.size
    # counter (site, shot, state, 0), key (low word, high word), u = ((x0 >> 5) 2^26 + (x1 >> 6)) 2^-53
    x = engine.philox4x32([4, 3, 2, 0], [11, 2**31])
    assert engine.sample_uniform(2**63 + 11, 2, 3, 4) == ((int(x[0]) >> 5) * 2**26 + (int(x[1]) >> 6)) * 2.0**-53
    b = engine.random_bases(40, 9, 5)
    assert b.shape == (40, 9) and b.dtype == np.uint8 and set(np.unique(b)) == {1, 2, 3}
    assert b[7, 3] == 1 + int(engine.philox4x32([3, 7, 0, 1], [5, 0])[0]) % 3
    assert np.array_equal(engine.random_bases(17, 9, 5), b[:17])  # a shorter table is the head of a longer one
    assert not np.array_equal(engine.random_bases(40, 9, 6), b)
    with pytest.raises(ValueError, match="seed"):
        engine.sample_uniform(-1, 0, 0, 0)


def test_mirror_probability_is_the_born_probability():
    states, dense = nine_qubit_case()
    bases = engine.random_bases(64, 9, 3)
    for i, (m, psi) in enumerate(zip(states, dense)):
        bits, lp = m.sample(64, bases=bases, seed=17, state_index=i, logp=True)
        assert bits.shape == (64, 9) and bits.dtype == np.uint8 and bits.max() <= 1
        # the state vector the MPS holds: 1e-8 relative for every drawn string
        exact = dense_probability(dense_of_mps(m), bits, bases)
        assert np.all(np.abs(np.exp(lp) - exact) <= 1e-8 * exact)
        # the state vector of the circuit, which the builder's truncation (error 1e-16: amplitudes to 1e-8) moved the MPS away from:
        # |dp| <= 2 sqrt(p) |d amplitude| <= 1e-8 absolute
        assert m.max_bond() >= 8 and np.abs(np.exp(lp) - dense_probability(psi, bits, bases)).max() <= 1e-8
    # the draws of two states differ, and so do two seeds
    a = states[0].sample(64, bases=bases, seed=17, state_index=0)
    assert not np.array_equal(a, states[0].sample(64, bases=bases, seed=18, state_index=0))
    assert not np.array_equal(a, states[0].sample(64, bases=bases, seed=17, state_index=1))
    # the first shots of a longer call are the shorter call
    assert np.array_equal(states[0].sample(17, bases=bases[:17], seed=17), states[0].sample(64, bases=bases, seed=17)[:17])


def test_mirror_does_not_see_the_norm():
    states, _ = nine_qubit_case()
    bases = engine.random_bases(64, 9, 3)
    for i, m in enumerate(states):
        bits, lp, margin = m.sample(64, bases=bases, seed=17, state_index=i, logp=True, margin=True)
        assert margin >= 1e-9  # no draw on a threshold: scaling may not flip one
        bits3, lp3 = Q.MPS([3.0 * t for t in m.tensors]).sample(64, bases=bases, seed=17, state_index=i, logp=True)
        assert np.array_equal(bits3, bits)
        assert np.abs(lp3 - lp).max() <= 1e-13


def test_bases_forms_and_rejections():
    states, _ = nine_qubit_case()
    m = states[0]
    z = m.sample(5, seed=2)
    assert np.array_equal(z, m.sample(5, bases="ZZZZZZZZZ", seed=2)) and np.array_equal(z, m.sample(5, bases=[3] * 9, seed=2))
    row = [1, 2, 3, 1, 2, 3, 1, 2, 3]
    assert np.array_equal(m.sample(5, bases="XYZXYZXYZ", seed=2), m.sample(5, bases=np.tile(row, (5, 1)), seed=2))
    for bad in ([0] * 9, [4] * 9, np.ones((5, 8), dtype=int), np.ones((4, 9), dtype=int), "ZZZ", "ZZZZZZZZI", np.ones(9)):
        with pytest.raises(ValueError, match="bases"):
            m.sample(5, bases=bad)
    with pytest.raises(ValueError, match="shots"):
        m.sample(0)
    with pytest.raises(ValueError, match="norm 0"):
        Q.MPS([0.0 * t for t in m.tensors]).sample(3)


def test_certain_outcomes():
    # H|0> on every qubit, X bases: every outcome is +1
    n = 5
    plus = Q.simulate(Q.BoundCircuit.from_gates(n, [("H", [q], []) for q in range(n)]), 1 - 1e-16)
    bits, lp = plus.sample(40, bases="X" * n, seed=1, logp=True)
    assert not bits.any() and np.abs(lp).max() < 1e-12
    # XXPhase(0.5) on |00>, Z bases: (|00> - i |11>)/sqrt2, both bits equal, each string with probability 1/2
    bell = Q.simulate(Q.BoundCircuit.from_gates(2, [("XXPhase", [0, 1], [0.5])]), 1 - 1e-16)
    bits, lp = bell.sample(200, seed=4, logp=True)
    assert np.array_equal(bits[:, 0], bits[:, 1]) and 0 < bits[:, 0].sum() < 200
    assert np.abs(np.exp(lp) - 0.5).max() < 1e-12
    # without the Hadamards the ansatz is Rz and XXPhase on |0..0>: only strings of even parity
    states, _ = ansatz_states(8, 2, 2, 5, hadamard_init=False)
    for i, m in enumerate(states):
        bits = m.sample(100, seed=9, state_index=i)
        assert not (bits.sum(axis=1) % 2).any() and bits.any()
    # Ry(alpha)|0>, Z basis: cos^2(pi alpha / 2) for bit 0, sin^2 for bit 1
    for alpha in (0.3, 0.5, 1.2):
        m = Q.simulate(Q.BoundCircuit.from_gates(1, [("Ry", [0], [alpha])]), 1 - 1e-16)
        bits, lp = m.sample(50, seed=3, logp=True)
        want = np.where(bits[:, 0] == 0, np.cos(np.pi * alpha / 2) ** 2, np.sin(np.pi * alpha / 2) ** 2)
        assert len(np.unique(bits)) == 2 and np.abs(np.exp(lp) - want).max() < 1e-12


def test_estimator_identities():
    # two states, four shots, three qubits, by hand
    bases = np.array([[1, 3, 3], [1, 3, 2], [2, 3, 3], [1, 1, 3]], dtype=np.uint8)
    bits = np.array([[[0, 1, 0], [1, 1, 0], [0, 0, 1], [0, 1, 1]], [[1, 1, 1], [1, 0, 0], [1, 0, 1], [1, 1, 0]]], dtype=np.uint8)
    F, counts = engine.estimate_paulis(bits, bases)
    assert F.shape == (2, 3, 3) and counts.shape == (3, 3)
    assert np.array_equal(counts, [[3, 1, 0], [1, 0, 3], [0, 1, 3]])
    assert np.array_equal(F[0], [[1 / 3, 1.0, 0.0], [-1.0, 0.0, -1 / 3], [0.0, 1.0, -1 / 3]])
    assert np.array_equal(F[1], [[-1.0, -1.0, 0.0], [-1.0, 0.0, 1 / 3], [0.0, 1.0, -1 / 3]])
    T = engine.estimate_pair_paulis(bits, bases, max_dist=2)
    assert T.shape == (2, 3, 4, 4) and np.all(T[:, :, 0, 0] == 1.0)
    pairs = engine.pair_table(3, 2)
    for pi, (a, b) in enumerate(pairs):
        assert np.array_equal(T[:, pi, 1:, 0], F[:, a]) and np.array_equal(T[:, pi, 0, 1:], F[:, b])
    # pair (0, 1): (X, Z) in shots 0 and 1, (Y, Z) in shot 2, (X, X) in shot 3; state 0 signs (+,-), (-,-), (+,+), (+,-)
    assert T[0, 0, 1, 3] == 0.0 and T[0, 0, 2, 3] == 1.0 and T[0, 0, 1, 1] == -1.0 and T[0, 0, 3, 3] == 0.0
    # pair (0, 2) is the third row: (X, Z) in shots 0 and 3: signs (+,+), (+,-)
    assert tuple(pairs[2]) == (0, 2) and T[0, 2, 1, 3] == 0.0 and T[1, 2, 1, 3] == 0.0 and T[1, 2, 1, 2] == -1.0
    # all outcomes +1: every measured entry is 1
    F1, _ = engine.estimate_paulis(np.zeros((1, 4, 3), dtype=np.uint8), bases)
    assert np.array_equal(F1[0], (counts > 0).astype(float))
    # a shared row and a string are tables
    assert np.array_equal(engine.estimate_paulis(bits, "XZZ")[0], engine.estimate_paulis(bits, np.tile([1, 3, 3], (4, 1)))[0])
    with pytest.raises(ValueError, match="bases"):
        engine.estimate_paulis(bits, np.zeros((4, 3), dtype=int))
    with pytest.raises(ValueError, match="bits"):
        engine.estimate_paulis(bits[0], bases)


def test_estimators_converge_on_mirror_shots():
    from test_projected_host import bloch_from_dense
    from test_projected_pair_host import pair_from_dense

    n, shots = 6, 4096
    states, circs = ansatz_states(n, 2, 1, 31)
    psi = dense_of_circuit(circs[0])
    F, _ = bloch_from_dense(psi, n)
    T, _ = pair_from_dense(psi, n)
    # the outcome is a function of the seed; seed 5 was chosen as one for which every entry lies inside 5 standard errors
    bases = engine.random_bases(shots, n, 5)
    bits = states[0].sample(shots, bases=bases, seed=5)[None]
    F_hat, counts = engine.estimate_paulis(bits, bases)
    assert counts.min() > shots / 4
    assert np.all(np.abs(F_hat[0] - F) <= 5.0 / np.sqrt(counts))
    T_hat = engine.estimate_pair_paulis(bits, bases)
    for k in range(n - 1):
        for p in range(1, 4):
            for q in range(1, 4):
                cnt = int(((bases[:, k] == p) & (bases[:, k + 1] == q)).sum())
                assert abs(T_hat[0, k, p, q] - T[k, p, q]) <= 5.0 / np.sqrt(cnt)


def test_symbol_is_declared():
    assert "qk_sample_host" in engine.EXPORTED_SYMBOLS
