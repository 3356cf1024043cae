"""CPU tier: the classical-shadow kernel's shot-pair histograms in numpy (engine.pack_shadow_words, shadow_hist, shadow_inner,
shadow_kernel).  Definitions (include/qkgram.h, README "Finite shots: the shadow kernel"): bit 0 = eigenvalue +1, codes 1, 2, 3 = X,
Y, Z; the single-qubit shadow of a shot is sigma = 3 |s><s| - I, tr(sigma_k sigma'_k) is 5, -4 or 1/2, so a shot pair enters through
d = (same basis, same outcome) - (same basis, other outcome) and sum_k tr(sigma_k sigma'_k) = n/2 + 4.5 d.  Every expected value here
is restated from 2 x 2 matrices or counted qubit by qubit, not taken from the mirror."""
import functools
import os

import numpy as np
import pytest

from qml_cutensornet_amd import engine
from test_sample_host import ansatz_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END_TO_END = {"n": 8, "layers": 2, "states": 4, "state_seed": 41, "shots": 48, "shot_seed": 3}

_S = np.sqrt(0.5)
# eigenvectors |s> of X, Y, Z for outcome bit 0 (eigenvalue +1) and 1
EIGVEC = {1: (np.array([_S, _S]), np.array([_S, -_S])), 2: (np.array([_S, 1j * _S]), np.array([_S, -1j * _S])), 3: (np.array([1.0, 0.0]), np.array([0.0, 1.0]))}


def sigma(code, bit):
    v = EIGVEC[int(code)][int(bit)]
    return 3.0 * np.outer(v, v.conj()) - np.eye(2)


def random_shots(rng, ns, shots, n, per_state=False):
    """(bits (ns, shots, n), bases (shots, n) or (ns, shots, n))"""
    bits = rng.integers(0, 2, size=(ns, shots, n), dtype=np.uint8)
    bases = rng.integers(1, 4, size=(ns, shots, n) if per_state else (shots, n), dtype=np.uint8)
    return bits, bases


def qubitwise_d(bits_a, bases_a, bits_b, bases_b):
    """d of two shots, counted qubit by qubit"""
    d = 0
    for k in range(len(bits_a)):
        if bases_a[k] == bases_b[k]:
            d += 1 if bits_a[k] == bits_b[k] else -1
    return d


def qubitwise_hist(bx, cx, by, cy, i, j, equal=False):
    n = bx.shape[2]
    H = np.zeros(2 * n + 1, dtype=np.int64)
    ci = cx[i] if cx.ndim == 3 else cx
    cj = cy[j] if cy.ndim == 3 else cy
    for t in range(bx.shape[1]):
        for u in ([t] if equal else range(by.shape[1])):
            H[qubitwise_d(bx[i, t], ci[t], by[j, u], cj[u]) + n] += 1
    return H


def upper_pairs(count):
    return np.stack(np.triu_indices(count), axis=1)


@functools.lru_cache(maxsize=None)
def end_to_end_case():
    """(states, bases table, bits (n_states, shots, n) of ``MPS.sample``) of END_TO_END"""
    c = END_TO_END
    states, _ = ansatz_states(c["n"], c["layers"], c["states"], c["state_seed"])
    B = engine.random_bases(c["shots"], c["n"], c["shot_seed"])
    bits = np.stack([m.sample(c["shots"], bases=B, seed=c["shot_seed"], state_index=s) for s, m in enumerate(states)])
    return states, B, bits


def test_trace_of_two_single_qubit_shadows_takes_three_values():
    for ca in (1, 2, 3):
        for cb in (1, 2, 3):
            for a in (0, 1):
                for b in (0, 1):
                    want = 0.5 if ca != cb else (5.0 if a == b else -4.0)
                    assert abs(np.trace(sigma(ca, a) @ sigma(cb, b)) - want) < 1e-12


def test_mirror_against_per_qubit_traces():
    rng = np.random.default_rng(0)
    for n, tx, ty, per_state in ((1, 3, 2, False), (4, 5, 3, True), (7, 4, 6, False), (33, 3, 3, True)):
        bx, cx = random_shots(rng, 2, tx, n, per_state)
        by, cy = random_shots(rng, 3, ty, n, per_state)
        pairs = [(0, 0), (1, 2), (0, 1), (1, 2)]
        H = engine.shadow_hist(bx, cx, by, cy, pairs)
        assert H.dtype == np.int64 and H.shape == (4, 2 * n + 1) and np.all(H.sum(axis=1) == tx * ty)
        for e, (i, j) in enumerate(pairs):
            assert np.array_equal(H[e], qubitwise_hist(bx, cx, by, cy, i, j))
        # sum_k tr(sigma_k sigma'_k) = n/2 + 4.5 d, from the 2 x 2 matrices, on the first pair
        ci, cj = (cx[0], cy[0]) if per_state else (cx, cy)
        total = sum(sum(np.trace(sigma(ci[t, k], bx[0, t, k]) @ sigma(cj[u, k], by[0, u, k])).real for k in range(n)) for t in range(tx) for u in range(ty))
        d = np.arange(-n, n + 1)
        assert abs(total - np.sum(H[0] * (0.5 * n + 4.5 * d))) < 1e-9 * max(1.0, abs(total))
        assert abs(engine.shadow_inner(H[0], n, weights=lambda dd: 0.5 * n + 4.5 * dd) - total / (tx * ty)) < 1e-12 * max(1.0, abs(total))


def test_equal_histograms():
    rng = np.random.default_rng(1)
    n, T = 6, 9
    bx, cx = random_shots(rng, 3, T, n)
    by, cy = random_shots(rng, 2, T, n, per_state=True)
    H, E = engine.shadow_hist(bx, cx, by, cy, [(2, 1), (0, 0)], equal=True)
    for e, (i, j) in enumerate([(2, 1), (0, 0)]):
        assert np.array_equal(E[e], qubitwise_hist(bx, cx, by, cy, i, j, equal=True)) and E[e].sum() == T
    assert np.all(H - E >= 0)
    # a self pair: a shot paired with itself has d = n
    H, E = engine.shadow_hist(bx, cx, None, None, [(1, 1), (0, 2)], equal=True)
    want = np.zeros(2 * n + 1, dtype=np.int64)
    want[2 * n] = T
    assert np.array_equal(E[0], want) and E[1].sum() == T
    # a shared table: the pairs t = t' share their bases on every qubit, so d has the parity of n and never leaves [-n, n]
    assert np.all(E[1][(np.arange(2 * n + 1) - n - n) % 2 == 1] == 0)


@pytest.mark.parametrize("per_state", [False, True])
def test_linear_weight_identity_with_estimate_paulis(per_state):
    """sum_d H f(d) / (T_x T_y) = sum_k (1 + r_k(x) . r_k(y)) / 2 with f(d) = n/2 + 4.5 d and r_k[c] = 3 counts_k[c] / T F_hat[k][c]"""
    rng = np.random.default_rng(2)
    n, tx, ty = 7, 13, 9
    bx, cx = random_shots(rng, 2, tx, n, per_state)
    by, cy = random_shots(rng, 2, ty, n, per_state)

    def r_of(bits, bases, s):
        F, counts = engine.estimate_paulis(bits[s : s + 1], bases[s] if bases.ndim == 3 else bases)
        return 3.0 * counts / bits.shape[1] * F[0]

    H = engine.shadow_hist(bx, cx, by, cy, [(0, 1), (1, 0)])
    for e, (i, j) in enumerate([(0, 1), (1, 0)]):
        want = np.sum(1.0 + np.sum(r_of(bx, cx, i) * r_of(by, cy, j), axis=1)) / 2.0
        got = engine.shadow_inner(H[e], n, weights=lambda d: 0.5 * n + 4.5 * d)
        assert abs(got - want) < 1e-12 * abs(want)


def test_known_answers():
    n, T = 9, 5
    rng = np.random.default_rng(3)
    row, codes = rng.integers(0, 2, size=n, dtype=np.uint8), rng.integers(1, 4, size=n, dtype=np.uint8)
    bits, bases = np.tile(row, (1, T, 1)), np.tile(codes, (T, 1))

    def only(bin_):
        want = np.zeros((1, 2 * n + 1), dtype=np.int64)
        want[0, bin_] = T * T
        return want

    assert np.array_equal(engine.shadow_hist(bits, bases, bits, bases, [(0, 0)]), only(2 * n))  # identical constant tables
    assert np.array_equal(engine.shadow_hist(bits, bases, 1 - bits, bases, [(0, 0)]), only(0))  # complemented outcomes
    assert np.array_equal(engine.shadow_hist(bits, np.full((T, n), 3), bits, np.full((T, n), 1), [(0, 0)]), only(n))  # all Z against all X


def test_pack_shadow_words():
    rng = np.random.default_rng(4)
    for n in (1, 31, 32, 33, 64, 65, 128):
        bits, bases = rng.integers(0, 2, size=(2, 3, n)), rng.integers(1, 4, size=(3, n))
        rec = engine.pack_shadow_words(bits, bases)
        assert rec.dtype == np.uint32 and rec.shape == (2, 3, (n + 31) // 32, 3)
        for k in range(32 * rec.shape[2]):
            got = (rec[:, :, k // 32, :] >> np.uint32(k % 32)) & np.uint32(1)
            if k < n:
                assert np.array_equal(got[..., 0], bits[..., k]) and np.array_equal(got[..., 1], np.broadcast_to(bases[:, k] & 1, (2, 3)))
                assert np.array_equal(got[..., 2], np.broadcast_to(bases[:, k] >> 1, (2, 3)))
            else:
                assert not got.any()  # pad bits are 0 in all planes
    good_bits, good_bases = np.zeros((2, 4), dtype=np.int64), np.full((2, 4), 3)
    for bits, bases, match in ((good_bits + 2, good_bases, "bits"), (good_bits - 1, good_bases, "bits"), (good_bits, good_bases * 0, "bases"), (good_bits, good_bases + 1, "bases"),
                               (np.zeros((1, 129), dtype=np.int64), np.ones((1, 129), dtype=np.int64), "128"), (good_bits, np.full((3, 4), 3), "broadcast")):
        with pytest.raises(ValueError, match=match):
            engine.pack_shadow_words(bits, bases)
    assert engine.SHADOW_MAX_QUBITS == 128


def test_rejections():
    rng = np.random.default_rng(5)
    bx, cx = random_shots(rng, 2, 3, 5)
    by, cy = random_shots(rng, 2, 4, 5)
    for args, kw, match in (
        ((bx, cx, None, cx, [(0, 1)]), {}, "bases_y"),
        ((bx, cx, by, None, [(0, 1)]), {}, "bases_y"),
        ((bx, cx[:2], None, None, [(0, 1)]), {}, "bases_x"),
        ((bx, cx, by, cy, [(0, 2)]), {}, "pairs"),
        ((bx, cx, by, cy, [(0, 1)]), {"equal": True}, "equal"),
        ((bx, cx, by[:, :, :4], cy[:, :4], [(0, 1)]), {}, "qubits"),
        ((bx + 2, cx, None, None, [(0, 1)]), {}, "bits"),
        ((bx, cx * 0, None, None, [(0, 1)]), {}, "bases"),
    ):
        with pytest.raises(ValueError, match=match):
            engine.shadow_hist(*args, **kw)
    H = engine.shadow_hist(bx, cx, None, None, [(0, 1)])
    with pytest.raises(ValueError, match="bins"):
        engine.shadow_inner(H, 4)
    with pytest.raises(ValueError, match="weights"):
        engine.shadow_inner(H, 5, weights=np.ones(5))


def test_inner_and_kernel_forms():
    rng = np.random.default_rng(6)
    n, T = 6, 10
    bx, cx = random_shots(rng, 3, T, n)
    pairs = upper_pairs(3)
    H, E = engine.shadow_hist(bx, cx, None, None, pairs, equal=True)
    d = np.arange(-n, n + 1)
    for gamma in (1.0, 0.3):
        w = np.exp(gamma / n * (0.5 * n + 4.5 * d))
        want = (H * w).sum(axis=1) / (T * T)
        assert np.allclose(engine.shadow_inner(H, n, gamma), want, rtol=1e-14, atol=0)
        assert np.array_equal(engine.shadow_inner(H, n, gamma), engine.shadow_inner(H, n, weights=w))
        assert np.array_equal(engine.shadow_inner(H, n, gamma), engine.shadow_inner(H, n, weights=lambda dd: np.exp(gamma / n * (0.5 * n + 4.5 * dd))))
        skip = ((H - E) * w).sum(axis=1) / (T * (T - 1))
        assert np.allclose(engine.shadow_inner(H, n, gamma, equal=E), skip, rtol=1e-14, atol=0)
        for tau in (1.0, 0.5):
            assert np.allclose(engine.shadow_kernel(H, n, gamma, tau), np.exp(tau * want), rtol=1e-14, atol=0)
            assert np.allclose(engine.shadow_kernel(H, n, gamma, tau, equal=E), np.exp(tau * skip), rtol=1e-14, atol=0)
    # any leading shape
    assert engine.shadow_kernel(H.reshape(2, 3, -1), n).shape == (2, 3)


def test_grams_are_positive_semidefinite():
    rng = np.random.default_rng(7)
    n, T, ns = 10, 12, 9
    bx, cx = random_shots(rng, ns, T, n, per_state=True)
    pairs = upper_pairs(ns)
    H = engine.shadow_hist(bx, cx, None, None, pairs)
    full = np.zeros((ns, ns, 2 * n + 1), dtype=np.int64)
    full[pairs[:, 0], pairs[:, 1]] = H
    full[pairs[:, 1], pairs[:, 0]] = H
    for G in (engine.shadow_inner(full, n), engine.shadow_kernel(full, n), engine.shadow_inner(full, n, gamma=0.2), engine.shadow_kernel(full, n, 0.2, 3.0)):
        ev = np.linalg.eigvalsh(G)
        assert np.array_equal(G, G.T) and ev[0] >= -1e-12 * ev[-1], ev


def test_end_to_end_on_ansatz_states():
    c = END_TO_END
    states, B, bits = end_to_end_case()
    n, T, ns = c["n"], c["shots"], c["states"]
    pairs = upper_pairs(ns)
    H, E = engine.shadow_hist(bits, B, None, None, pairs, equal=True)
    assert np.all(H.sum(axis=1) == T * T) and np.all(E.sum(axis=1) == T)
    for e in (1, 5):
        i, j = pairs[e]
        assert np.array_equal(H[e], qubitwise_hist(bits, B, bits, B, i, j))
    # the first-order term is the shot-noise one-qubit projected kernel's inner product
    F, counts = engine.estimate_paulis(bits, B)
    r = 3.0 * counts / T * F
    lin = engine.shadow_inner(H, n, weights=lambda d: 0.5 * n + 4.5 * d)
    for e, (i, j) in enumerate(pairs):
        assert abs(lin[e] - np.sum(1.0 + np.sum(r[i] * r[j], axis=1)) / 2.0) < 1e-12 * abs(lin[e])
    K = engine.shadow_kernel(H, n)
    assert np.all(np.isfinite(K)) and np.all(K > 1.0)
    # with every shot pair, inner is an inner product of mean feature vectors: |m_i - m_j|^2 = inner_ii + inner_jj - 2 inner_ij >= 0
    inner = dict(zip(map(tuple, pairs), engine.shadow_inner(H, n)))
    for (i, j), v in inner.items():
        assert inner[(i, i)] + inner[(j, j)] - 2.0 * v >= -1e-12 * v


def test_header_and_bindings_declare_the_symbol():
    with open(os.path.join(ROOT, "include", "qkgram.h")) as fp:
        header = fp.read()
    assert "int qk_shadow_hist_host(qk_ctx* ctx, int32_t n_sites," in header
    assert any(name == "qk_shadow_hist_host" and len(args) == 16 for name, _, args in engine._SIGNATURES)
