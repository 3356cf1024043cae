"""Pauli strings and window RDMs estimated from measurement shots, on the host (no GPU): the numpy mirror ``engine.shot_string_sums``
against a table worked by hand and a loop over the qubits, the identities that tie it to ``estimate_paulis`` and
``estimate_pair_paulis`` (equal as floats), the order of ``window_strings`` against ``MPS.window_rdm``, the designed bases of
``window_settings``, convergence on mirror shots, the semantics of the estimated window RDMs, and the rejections."""
import functools
import os

import numpy as np
import pytest

from qml_cutensornet_amd import engine
from test_pauli_strings_host import pair_strings, pauli_strings_from_dense, weight_one_strings
from test_sample_host import ansatz_states, dense_of_circuit, dense_of_mps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def loop_sums(bits, bases, strings):
    """(sums, counts) by the definition: a loop over states, strings, shots and qubits."""
    bits, bases, strings = np.asarray(bits), np.asarray(bases), np.asarray(strings)
    ns, T, n = bits.shape
    sums, counts = np.zeros((ns, len(strings)), dtype=np.int64), np.zeros((ns, len(strings)), dtype=np.int64)
    for s in range(ns):
        B = bases[s] if bases.ndim == 3 else bases
        for m, c in enumerate(strings):
            for t in range(T):
                sign, match = 1, True
                for k in range(n):
                    if c[k]:
                        match = match and B[t, k] == c[k]
                        sign *= 1 - 2 * int(bits[s, t, k])
                if match:
                    counts[s, m] += 1
                    sums[s, m] += sign
    return sums, counts


def random_case(rng, ns, T, n, m, per_state):
    """Random bits and bases and m strings: the identity first, a full-weight string second (it matches shot 0 of state 0), a
    duplicate of a sparse string last, sparse strings that agree with some shot's bases between."""
    bits = rng.integers(0, 2, (ns, T, n), dtype=np.uint8)
    bases = rng.integers(1, 4, (ns, T, n) if per_state else (T, n), dtype=np.uint8)
    rows = bases.reshape(-1, n)
    S = np.zeros((m, n), dtype=np.uint8)
    for j in range(m):
        if j == 1:
            S[j] = rows[0]
        elif j >= 2:
            keep = rng.random(n) < min(1.0, 3.0 / n)
            S[j] = np.where(keep, rows[rng.integers(len(rows))] if j % 3 else rng.integers(1, 4, n), 0)
    if m > 3:
        S[-1] = S[2]
    return bits, bases, S


@functools.lru_cache(maxsize=None)
def six_qubit_shots():
    """One 6-qubit, 2-layer ansatz state, its dense vector, and its mirror shots at seed 5: 4 096 in random bases, 27 * 128 in the
    designed bases of width 3.  Computed once, shared, left unchanged."""
    states, circs = ansatz_states(6, 2, 1, 31)
    rb = engine.random_bases(4096, 6, 5)
    wb = engine.window_settings(27 * 128, 6, 3)
    out = {"psi": dense_of_circuit(circs[0]), "mps": states[0], "random": (states[0].sample(4096, bases=rb, seed=5)[None], rb),
           "window": (states[0].sample(27 * 128, bases=wb, seed=5)[None], wb)}
    for b, c in (out["random"], out["window"]):
        b.setflags(write=False), c.setflags(write=False)
    return out


def test_table_by_hand():
    # the table of test_estimator_identities: two states, four shots, three qubits
    bases = np.array([[1, 3, 3], [1, 3, 2], [2, 3, 3], [1, 1, 3]], dtype=np.uint8)
    bits = np.array([[[0, 1, 0], [1, 1, 0], [0, 0, 1], [0, 1, 1]], [[1, 1, 1], [1, 0, 0], [1, 0, 1], [1, 1, 0]]], dtype=np.uint8)
    strings = ["III", "XII", "IZI", "XZI", "XZZ", "YZZ", "ZZZ", "IIZ", ("XZ", (0, 2))]
    sums, counts = engine.shot_string_sums(bits, bases, strings)
    #   III: every shot, sign +1.  XII: shots 0, 1, 3.  IZI: shots 0, 1, 2.  XZI: shots 0, 1.  XZZ: shot 0.  YZZ: shot 2.  ZZZ: none.
    #   IIZ: shots 0, 2, 3.  X on 0 and Z on 2: shots 0, 3.
    assert np.array_equal(counts, [[4, 3, 3, 2, 1, 1, 0, 3, 2]] * 2)
    # state 0 signs per shot (qubit 0, 1, 2): (+,-,+), (-,-,+), (+,+,-), (+,-,-)
    assert np.array_equal(sums[0], [4, 1, -1, 0, -1, -1, 0, -1, 0])
    # state 1: (-,-,-), (-,+,+), (-,+,-), (-,-,+)
    assert np.array_equal(sums[1], [4, -3, 1, 0, -1, 1, 0, -1, 0])
    vals = engine.string_values(sums, counts)
    assert vals.dtype == np.float64 and np.array_equal(vals[0], [1.0, 1 / 3, -1 / 3, 0.0, -1.0, -1.0, 0.0, -1 / 3, 0.0])
    assert vals[0, 6] == 0.0 and counts[0, 6] == 0  # no shot: 0.0, the convention of estimate_paulis
    # bases per state: state 1 measured in other bases
    per = np.stack([bases, bases[::-1]])
    s2, c2 = engine.shot_string_sums(bits, per, strings)
    assert np.array_equal(s2[0], sums[0]) and np.array_equal(c2[0], counts[0])
    assert np.array_equal((s2[1], c2[1]), [a[0] for a in engine.shot_string_sums(bits[1:], bases[::-1], strings)])
    assert np.array_equal(c2[1], counts[1]) and not np.array_equal(s2[1], sums[1])


@pytest.mark.parametrize("n", [1, 31, 32, 33, 65, 128])
@pytest.mark.parametrize("per_state", [False, True])
def test_mirror_against_a_loop_over_the_qubits(n, per_state):
    rng = np.random.default_rng(100 * n + per_state)
    bits, bases, S = random_case(rng, 2, 9, n, 8, per_state)
    sums, counts = engine.shot_string_sums(bits, bases, S)
    want_s, want_c = loop_sums(bits, bases, S)
    assert sums.dtype == np.int64 and counts.dtype == np.int64
    assert np.array_equal(sums, want_s) and np.array_equal(counts, want_c)
    assert np.all(counts[:, 0] == 9) and np.all(sums[:, 0] == 9)  # the identity
    assert counts[0, 1] >= 1  # the full-weight string matches the shot it was copied from
    assert np.array_equal(sums[:, -1], sums[:, 2]) and np.array_equal(counts[:, -1], counts[:, 2])  # duplicates
    assert counts[:, 2:].max() >= 1 and (n == 1 or counts[:, 1:].min() < 9)
    # a (state, string) result does not depend on the other states or strings
    sub_s, sub_c = engine.shot_string_sums(bits[1:], bases[1:] if per_state else bases, S[[5, 1]])
    assert np.array_equal(sub_s[0], sums[1, [5, 1]]) and np.array_equal(sub_c[0], counts[1, [5, 1]])


def test_weight_one_and_pair_strings_are_the_older_estimators():
    n = 6
    bits, bases = six_qubit_shots()["random"]
    F, _ = engine.estimate_paulis(bits, bases)
    V = engine.string_values(*engine.shot_string_sums(bits, bases, weight_one_strings(n)))
    assert np.array_equal(V.reshape(1, n, 3), F)
    T = engine.estimate_pair_paulis(bits, bases, max_dist=2)
    V2 = engine.string_values(*engine.shot_string_sums(bits, bases, pair_strings(n, 2))).reshape(1, -1, 4, 4)
    assert np.array_equal(V2[:, :, 1:, 1:], T[:, :, 1:, 1:])
    assert np.array_equal(V2, T)  # the identity and the one-qubit rows and columns too


@pytest.mark.parametrize("n,width,starts", [(6, 1, None), (6, 2, None), (6, 3, None), (7, 3, [0, 2, 3, 4]), (6, 6, None), (7, 4, [1, 3])])
def test_window_strings_order(n, width, starts):
    states, _ = ansatz_states(n, 2, 2, 17)  # (the dense vector of the MPS itself: the builder's truncation is not under test)
    S = engine.window_strings(n, width, starts)
    st = list(range(n - width + 1)) if starts is None else starts
    assert S.shape == (len(st) * 4 ** width, n) and S.dtype == np.uint8
    vals = np.stack([pauli_strings_from_dense(dense_of_mps(m), n, S)[0] for m in states]).reshape((2, len(st)) + (4,) * width)
    rho = engine.paulis_rdm(vals, width=width)
    assert rho.shape == (2, len(st), 1 << width, 1 << width)
    for s, m in enumerate(states):
        for i, a in enumerate(st):
            assert np.abs(rho[s, i] - m.window_rdm(a, width)).max() < 1e-12
    # and back: the coefficients of the exact window RDMs are the values, in this order
    assert np.abs(engine.rdm_paulis(rho) - vals).max() < 1e-12


@pytest.mark.parametrize("n,width,rounds", [(7, 1, 5), (7, 2, 3), (8, 3, 2), (9, 4, 1), (6, 6, 1)])
def test_window_settings_counts(n, width, rounds):
    shots = rounds * 3 ** width
    bases = engine.window_settings(shots, n, width)
    assert bases.shape == (shots, n) and bases.dtype == np.uint8 and bases.min() >= 1 and bases.max() <= 3
    t = np.arange(shots) % 3 ** width
    for k in range(n):
        assert np.array_equal(bases[:, k], 1 + (t // 3 ** (k % width)) % 3)
    S = engine.window_strings(n, width)
    _, counts = engine.shot_string_sums(np.zeros((1, shots, n), dtype=np.uint8), bases, S)
    weight = (S != 0).sum(axis=1)
    assert np.array_equal(counts[0] * 3 ** weight, np.full(len(S), shots))
    assert np.array_equal(engine.window_settings(shots + 5, n, width)[:shots], bases)


@pytest.mark.parametrize("which", ["window", "random"])
def test_estimates_converge_on_mirror_shots(which):
    """The bound of test_estimators_converge_on_mirror_shots, 5 standard errors, on all 4 x 64 strings of the width-3 windows.  The
    outcome is a function of the seed: with the mirror sampler at seed 5 the largest deviation is 2.66 standard errors in the
    designed bases and 2.76 in random ones."""
    case = six_qubit_shots()
    bits, bases = case[which]
    S = engine.window_strings(6, 3)
    assert len(S) == 4 * 64
    exact, _ = pauli_strings_from_dense(case["psi"], 6, S)
    sums, counts = engine.shot_string_sums(bits, bases, S)
    vals = engine.string_values(sums, counts)[0]
    dev = np.abs(vals - exact) * np.sqrt(counts[0])
    print(f"{which}: least count {counts.min()}, largest deviation {dev.max():.3f} standard errors")
    assert counts.min() >= 100
    assert np.all(np.abs(vals - exact) <= 5.0 / np.sqrt(counts[0]))


def test_estimated_window_rdms_semantics():
    bits, bases = six_qubit_shots()["random"]
    sigma = np.array([[[0, 1], [1, 0]], [[0, -1j], [1j, 0]], [[1, 0], [0, -1]]])
    for width in (1, 2, 3):
        rho, counts = engine.estimate_window_rdms(bits, bases, width)
        nw, D = 6 - width + 1, 1 << width
        assert rho.shape == (1, nw, D, D) and rho.dtype == np.complex128 and counts.shape == (1, nw) + (4,) * width
        assert np.array_equal(rho, np.conj(np.swapaxes(rho, -1, -2)))  # exactly Hermitian
        assert np.array_equal(np.trace(rho, axis1=-2, axis2=-1), np.ones((1, nw)))  # trace exactly 1
        assert np.all(counts[(0, slice(None)) + (0,) * width] == 4096)  # the identity sees every shot
        vals = engine.string_values(*engine.shot_string_sums(bits, bases, engine.window_strings(6, width)))
        assert np.array_equal(rho, engine.paulis_rdm(vals.reshape((1, nw) + (4,) * width), width=width))
    rho1, _ = engine.estimate_window_rdms(bits, bases, 1)
    F, _ = engine.estimate_paulis(bits, bases)
    want = (np.eye(2)[None, None] + np.einsum("skc,cab->skab", F, sigma)) / 2
    assert np.abs(rho1 - want).max() < 1e-15
    # chosen windows are the rows of the full call
    some, _ = engine.estimate_window_rdms(bits, bases, 3, starts=[1, 3])
    assert np.array_equal(some, engine.estimate_window_rdms(bits, bases, 3)[0][:, [1, 3]])
    # few shots: still Hermitian with trace 1, but not positive
    few, _ = engine.estimate_window_rdms(bits[:, :40], bases[:40], 3)
    assert np.array_equal(few, np.conj(np.swapaxes(few, -1, -2))) and np.abs(np.trace(few, axis1=-2, axis2=-1) - 1).max() < 1e-15
    assert np.linalg.eigvalsh(few).min() < -1e-3


def test_rejections_by_name():
    bits = np.zeros((2, 4, 3), dtype=np.uint8)
    bases = np.full((4, 3), 3, dtype=np.uint8)
    for bad_bits in (bits[0], bits.astype(float), np.zeros((0, 4, 3), dtype=np.uint8), np.zeros((2, 0, 3), dtype=np.uint8)):
        with pytest.raises(ValueError, match="bits"):
            engine.shot_string_sums(bad_bits, bases, ["ZZZ"])
    for bad_bases in (bases[:3], bases[:, :2], bases.astype(float), np.stack([bases] * 3)):
        with pytest.raises(ValueError, match="bases"):
            engine.shot_string_sums(bits, bad_bases, ["ZZZ"])
    with pytest.raises(ValueError, match="bases"):
        engine.shot_string_sums(bits, np.zeros((4, 3), dtype=np.uint8), ["ZZZ"])  # code 0 is no basis
    with pytest.raises(ValueError, match="bits"):
        engine.shot_string_sums(bits + 2, bases, ["ZZZ"])
    with pytest.raises(ValueError, match="ZZ"):
        engine.shot_string_sums(bits, bases, ["ZZ"])
    with pytest.raises(ValueError, match="empty"):
        engine.shot_string_sums(bits, bases, [])
    with pytest.raises(ValueError, match=r"strings\[1\]"):
        engine.shot_string_sums(bits, bases, np.array([[0, 1, 2], [0, 4, 0]]))
    with pytest.raises(ValueError, match="strings"):
        engine.shot_string_sums(bits, bases, np.zeros((2, 4), dtype=np.uint8))
    with pytest.raises(ValueError, match="128"):
        engine.shot_string_sums(np.zeros((1, 2, 129), dtype=np.uint8), np.full((2, 129), 3, dtype=np.uint8), np.zeros((1, 129), dtype=np.uint8))
    with pytest.raises(ValueError, match="sums and counts"):
        engine.string_values(np.zeros((2, 3), dtype=np.int64), np.zeros((2, 2), dtype=np.int64))
    with pytest.raises(ValueError, match="sums and counts"):
        engine.string_values(np.zeros((2, 3)), np.zeros((2, 3), dtype=np.int64))
    for width in (0, 7, 4, True, 2.0):
        with pytest.raises(ValueError, match="width"):
            engine.window_strings(3, width)
        with pytest.raises(ValueError, match="width"):
            engine.window_settings(9, 3, width)
        with pytest.raises(ValueError, match="width"):
            engine.estimate_window_rdms(bits, bases, width)
    for starts in ([], [2], [1, 0], [0, 0], [0.5], [-1]):
        with pytest.raises(ValueError, match="starts"):
            engine.window_strings(3, 2, starts)
    for shots in (0, -3, True, 2.5):
        with pytest.raises(ValueError, match="shots"):
            engine.window_settings(shots, 3, 2)


def test_symbol_is_declared():
    with open(os.path.join(ROOT, "include", "qkgram.h")) as fp:
        header = fp.read()
    assert "int qk_shot_strings_host(qk_ctx* ctx, int32_t n_sites, int32_t n_states, int32_t shots," in header
    assert "qk_shot_strings_host" in engine.EXPORTED_SYMBOLS
    assert any(name == "qk_shot_strings_host" and len(args) == 11 for name, _, args in engine._SIGNATURES)
    with open(os.path.join(ROOT, "qml-cutensornet_amd", "csrc", "qk_local_plan.h")) as fp:
        assert "QK_HD inline void sst_pack_string(" in fp.read()
