"""Block overlaps at finite shots on the host (no GPU): the randomised-measurement estimator of Elben et al., PRL 124, 010504 (2020),
as ``engine.shot_block_sums`` computes it -- the identity it rests on (its mean over all Pauli settings, on exact outcome
probabilities, is tr(rho_A rho'_A) for every width and both sides), known answers of the integer sums, convergence on shots of
ansatz states within four standard errors, the per-setting sums, ``setting_bases``, the packing, the rejections and the header.

Definitions (README "Finite shots: block overlaps", include/qkgram.h).  U settings of M shots; shot u M + a is shot a of setting u.
Packed word: side left, bit k = bits[k]; side right, bit k = bits[n-1-k]; k < min(n, 32).
    D_w(s, s')  = popcount((s xor s') & (2^w - 1))
    term_w      = (-1)^D_w 2^(w - D_w)
    S_u[w][p]   = sum_{a,b < M} term_w(X[i][uM+a], Y[j][uM+b])  -  [p is a self pair] M 2^w
    sums[w][p]  = sum_u S_u[w][p]
    N           = M^2 (cross pair), M (M - 1) (self pair: Y is X and i == j)
    O^_w        = sums / (U N),     stderr_w = std over u of S_u / N (ddof = 1) / sqrt(U)"""
import functools
import itertools
import os

import numpy as np
import pytest

from qml_cutensornet_amd import engine
from test_sample_host import OUTCOME_ROWS, ansatz_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDES = ("left", "right")
# The convergence cases.  The shot seeds were chosen on the CPU so that the numpy mirror satisfies |O^ - O| <= 4 stderr for every
# (pair, width, side): the standard error of a few settings is itself noisy, so not every seed does.  The device computes the same
# integers, so it inherits the choice.
CONVERGENCE = {"n": 8, "layers": 2, "states": 3, "state_seed": 31, "settings": 64, "shots_per_setting": 16, "shot_seed": 1}
END_TO_END = {"n": 12, "layers": 2, "states": 4, "state_seed": 32, "settings": 8, "shots_per_setting": 16, "shot_seed": 13}


@functools.lru_cache(maxsize=None)
def shot_case(name):
    """(states, bases table, bits (n_states, U M, n) of ``MPS.sample``) of CONVERGENCE or END_TO_END"""
    c = {"convergence": CONVERGENCE, "end_to_end": END_TO_END}[name]
    states, _ = ansatz_states(c["n"], c["layers"], c["states"], c["state_seed"])
    U, M = c["settings"], c["shots_per_setting"]
    B = engine.setting_bases(U, M, c["n"], c["shot_seed"])
    bits = np.stack([m.sample(U * M, bases=B, seed=c["shot_seed"], state_index=s) for s, m in enumerate(states)])
    return states, B, bits


def upper_pairs(count):
    iu = np.triu_indices(count)
    return np.stack(iu, axis=1)


def exact_block_overlaps(states, pairs, widths, side):
    return np.array([[states[i].block_overlap(states[j], int(w), side) for i, j in pairs] for w in widths])


def within_four_stderr(O_hat, stderr, exact):
    """every case: |O^ - O| <= 4 stderr (a standard error of 0 wants the exact value)"""
    return bool(np.all(np.isfinite(stderr)) and np.all(np.abs(O_hat - exact) <= 4.0 * stderr))


def random_tables(rng, ns, U, M, n):
    return rng.integers(0, 2, size=(ns, U * M, n), dtype=np.uint8)


def dense_reduced_overlap(psi, phi, w, side):
    n = psi.ndim
    def rho(v):
        m = v.reshape(2 ** w, 2 ** (n - w)) if side == "left" else v.reshape(2 ** (n - w), 2 ** w).T
        return m @ m.conj().T / np.vdot(v, v).real
    return float(np.trace(rho(psi) @ rho(phi)).real)


def outcome_probabilities(psi, setting):
    """Born probabilities of all 2^n strings (flat index = bits as a big-endian number over qubits 0 .. n-1) in the bases ``setting``"""
    amp = psi
    for k, c in enumerate(setting):
        amp = np.moveaxis(np.tensordot(OUTCOME_ROWS[int(c)], amp, axes=(1, k)), 0, k)
    p = np.abs(amp.reshape(-1)) ** 2
    return p / p.sum()


def test_identity_mean_over_all_settings_is_the_reduced_overlap():
    n = 4
    rng = np.random.default_rng(5)
    strings = np.array(list(itertools.product((0, 1), repeat=n)), dtype=np.uint8)  # row s = the bits of flat index s
    all_pairs = np.array([(s, t) for s in range(2 ** n) for t in range(2 ** n)])
    widths = [1, 2, 3, 4]
    for trial in range(3):
        psi, phi = (rng.normal(size=(2,) * n) + 1j * rng.normal(size=(2,) * n) for _ in range(2))
        for side in SIDES:
            # term_w(s, s') for every pair of strings: the estimator on tables of one shot
            terms = engine.shot_block_sums(strings[:, None, :], strings[:, None, :], 1, all_pairs, widths, side).reshape(len(widths), 2 ** n, 2 ** n)
            mean = np.zeros(len(widths))
            for setting in itertools.product((1, 2, 3), repeat=n):
                p, q = outcome_probabilities(psi, setting), outcome_probabilities(phi, setting)
                mean += np.einsum("s,wst,t->w", p, terms.astype(np.float64), q)
            mean /= 3 ** n
            for wi, w in enumerate(widths):
                assert abs(mean[wi] - dense_reduced_overlap(psi, phi, w, side)) <= 1e-12, (trial, side, w)


@pytest.mark.parametrize("side", SIDES)
def test_known_answers(side):
    rng = np.random.default_rng(7)
    U, M, n = 3, 5, 9
    widths = [1, 2, 8, 9]
    one = random_tables(rng, 1, U, 1, n)
    same = np.repeat(one, M, axis=1)  # (1, U M, n): every shot of a setting the same string
    both = np.concatenate([same, same])
    sums = engine.shot_block_sums(both, both, U, [(0, 1)], widths, side)
    assert sums.dtype == np.int64 and [int(v) for v in sums[:, 0]] == [U * M * M * 2 ** w for w in widths]
    sums = engine.shot_block_sums(both, None, U, [(0, 1), (1, 1)], widths, side)
    assert [int(v) for v in sums[:, 0]] == [U * M * M * 2 ** w for w in widths]
    assert [int(v) for v in sums[:, 1]] == [U * M * (M - 1) * 2 ** w for w in widths]
    sums = engine.shot_block_sums(same, 1 - same, U, [(0, 0)], widths, side)
    assert [int(v) for v in sums[:, 0]] == [(-1) ** w * U * M * M for w in widths]


def test_known_answer_beyond_32_bits():
    U, M, n = 3, 130, 33
    bits = np.repeat(random_tables(np.random.default_rng(8), 1, U, 1, n), M, axis=1)
    for side in SIDES:
        sums = engine.shot_block_sums(bits, bits, U, [(0, 0)], [31, 32], side)
        assert [int(v) for v in sums[:, 0]] == [U * M * M * 2 ** 31, U * M * M * 2 ** 32] and int(sums[1, 0]) > 2 ** 32


def test_convergence_within_four_standard_errors():
    c = CONVERGENCE
    states, _, bits = shot_case("convergence")
    U, M = c["settings"], c["shots_per_setting"]
    pairs = upper_pairs(len(states))
    widths = np.arange(1, c["n"] + 1)
    for side in SIDES:
        sums, S = engine.shot_block_sums(bits, None, U, pairs, widths, side, per_setting=True)
        O_hat, stderr = engine.shot_block_estimate(sums, S, U, M, pairs[:, 0] == pairs[:, 1])
        exact = exact_block_overlaps(states, pairs, widths, side)
        assert O_hat.shape == stderr.shape == exact.shape == (len(widths), len(pairs))
        assert within_four_stderr(O_hat, stderr, exact), (side, np.abs(O_hat - exact) / stderr)
        # the estimate says something: the narrow blocks are within 0.2 of the exact values
        assert np.max(np.abs(O_hat[:3] - exact[:3])) < 0.2


def test_end_to_end_case_satisfies_the_condition_on_the_mirror():
    c = END_TO_END
    states, _, bits = shot_case("end_to_end")
    pairs = upper_pairs(len(states))
    widths = np.arange(1, c["n"] + 1)
    for side in SIDES:
        sums, S = engine.shot_block_sums(bits, None, c["settings"], pairs, widths, side, per_setting=True)
        O_hat, stderr = engine.shot_block_estimate(sums, S, c["settings"], c["shots_per_setting"], pairs[:, 0] == pairs[:, 1])
        assert within_four_stderr(O_hat, stderr, exact_block_overlaps(states, pairs, widths, side)), side


def test_per_setting_adds_up_and_estimate():
    rng = np.random.default_rng(9)
    U, M, n = 5, 7, 6
    bx, by = random_tables(rng, 3, U, M, n), random_tables(rng, 2, U, M, n)
    pairs = [(2, 1), (0, 0), (2, 1), (1, 0)]
    sums, S = engine.shot_block_sums(bx, by, U, pairs, [1, 3, 6], "right", per_setting=True)
    assert S.shape == (3, 4, U) and S.dtype == np.int64 and np.array_equal(S.sum(axis=2), sums)
    assert np.array_equal(sums[:, 0], sums[:, 2])  # a duplicate pair
    assert np.array_equal(sums, engine.shot_block_sums(bx, by, U, pairs, [1, 3, 6], "right"))
    # one setting alone is that setting's S_u
    u = 3
    alone = engine.shot_block_sums(bx[:, u * M:(u + 1) * M], by[:, u * M:(u + 1) * M], 1, pairs, [1, 3, 6], "right")
    assert np.array_equal(alone, S[:, :, u])
    # a self pair: the a == b terms (each 2^w) are removed
    s_sym, S_sym = engine.shot_block_sums(bx, None, U, [(1, 1), (1, 2)], [2], "left", per_setting=True)
    s_rect = engine.shot_block_sums(bx, bx, U, [(1, 1), (1, 2)], [2], "left")
    assert int(s_rect[0, 0] - s_sym[0, 0]) == U * M * 4 and s_rect[0, 1] == s_sym[0, 1]
    O_hat, stderr = engine.shot_block_estimate(s_sym, S_sym, U, M, [True, False])
    assert O_hat[0, 0] == s_sym[0, 0] / (U * M * (M - 1)) and O_hat[0, 1] == s_sym[0, 1] / (U * M * M)
    want = np.std(S_sym[0, 1] / (M * M), ddof=1) / np.sqrt(U)
    assert abs(stderr[0, 1] - want) <= 1e-15 and stderr.shape == (1, 2)
    assert np.all(np.isnan(engine.shot_block_estimate(s_sym, None, U, M, [True, False])[1]))
    assert np.all(np.isnan(engine.shot_block_estimate(alone, alone[..., None], 1, M, False)[1]))


def test_setting_bases():
    B = engine.setting_bases(5, 3, 7, seed=11)
    assert B.shape == (15, 7) and B.dtype == np.uint8
    assert np.array_equal(B, np.repeat(engine.random_bases(5, 7, 11), 3, axis=0))
    assert np.array_equal(engine.setting_bases(5, 1, 7, 11), engine.random_bases(5, 7, 11))
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="shots_per_setting"):
            engine.setting_bases(5, bad, 7)


def test_pack_block_words():
    rng = np.random.default_rng(10)
    for n in (1, 5, 32, 33, 40):
        bits = rng.integers(0, 2, size=(2, 3, n), dtype=np.uint8)
        for side in SIDES:
            words = engine.pack_block_words(bits, side)
            assert words.shape == (2, 3) and words.dtype == np.uint32
            for k in range(32):
                want = (bits[..., k] if side == "left" else bits[..., n - 1 - k]) if k < min(n, 32) else 0
                assert np.all(((words >> np.uint32(k)) & np.uint32(1)) == want)
    bits = np.zeros((1, 1, 33), dtype=np.uint8)
    bits[0, 0, 32] = 2
    assert engine.pack_block_words(bits, "left")[0, 0] == 0  # qubit 32 is outside the left block
    with pytest.raises(ValueError, match="0 or 1"):
        engine.pack_block_words(bits, "right")


def test_rejections():
    rng = np.random.default_rng(12)
    bx = random_tables(rng, 2, 2, 3, 5)
    ok = dict(bits_x=bx, bits_y=None, settings=2, pairs=[(0, 1)], widths=[1, 5], side="left")
    assert engine.shot_block_sums(**ok).shape == (2, 1)
    for change, match in (
        (dict(bits_x=bx[0]), "bits_x"),
        (dict(bits_y=bx[:, :4]), "bits_y"),
        (dict(settings=4), "settings"),
        (dict(settings=0), "settings"),
        (dict(pairs=[(0, 2)]), "pairs"),
        (dict(pairs=[(-1, 0)]), "pairs"),
        (dict(widths=[0, 1]), "widths"),
        (dict(widths=[2, 2]), "widths"),
        (dict(widths=[6]), "widths"),
        (dict(widths=[]), "widths"),
        (dict(side="middle"), "side"),
        (dict(bits_x=bx + 2), "0 or 1"),
    ):
        with pytest.raises(ValueError, match=match):
            engine.shot_block_sums(**{**ok, **change})
    with pytest.raises(ValueError, match="shots_per_setting >= 2"):
        engine.shot_block_sums(bx, None, 6, [(1, 1)], [1])
    # widths stop at 32 however many qubits
    wide = random_tables(rng, 1, 1, 2, 40)
    with pytest.raises(ValueError, match="widths"):
        engine.shot_block_sums(wide, None, 1, [(0, 0)], [33])
    # the overflow rule: U M^2 2^w_max <= 2^62
    big = np.zeros((1, 2 ** 15 + 1, 32), dtype=np.uint8)
    with pytest.raises(ValueError, match="2\\^62"):
        engine.shot_block_sums(big, None, 1, [], [32])
    assert engine.shot_block_sums(big[:, : 2 ** 15], None, 1, [], [32]).shape == (1, 0)


def test_block_kernel_takes_estimates_as_they_are():
    O = np.array([[[0.9, 0.2], [0.2, -0.1]]])
    S = np.array([[0.9, -0.1]])
    K = engine.block_kernel(O, S, form="normalized")
    assert K[0, 0, 0] == 1.0 and K[0, 1, 1] == 1.0 and np.isnan(K[0, 0, 1]) and np.isnan(K[0, 1, 0])
    assert np.all(np.isfinite(engine.block_kernel(O, S, form="rbf")))


def test_header_and_bindings_declare_the_symbol():
    with open(os.path.join(ROOT, "include", "qkgram.h")) as fp:
        header = fp.read()
    assert "int qk_shot_block_sums_host(qk_ctx* ctx, int32_t n_sites, int32_t n_settings, int32_t shots_per_setting," in header
    assert "qk_shot_block_sums_host" in engine.EXPORTED_SYMBOLS
    for line in ("D_w(s, s')  = popcount((s xor s') & (2^w - 1))", "term_w      = (-1)^D_w 2^(w - D_w)", "U M^2 2^w_max <= 2^62"):
        assert line in header, line


@pytest.mark.parametrize(
    "n,kwargs,match",
    [
        (40, {"shots": (8, 16), "widths": (1, 33)}, "widths stop"),
        (40, {"shots": (8, 16), "widths": None}, "widths stop"),
        (4, {"shots": 8}, "shots"),
        (4, {"shots": (8,)}, "shots"),
        (4, {"shots": (0, 4)}, "shots"),
        (4, {"shots": (4, True)}, "shots"),
        (4, {"shots": (4, 2.0)}, "shots"),
        (4, {"shots": (4, 1)}, "shots_per_setting >= 2"),
    ],
)
def test_build_block_kernel_matrices_shot_argument_errors(monkeypatch, n, kwargs, match):
    import qml_cutensornet_amd as Q
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend import kernel_state_ansatz as K

    def no_device(*a, **k):
        raise AssertionError("device work before the argument checks")

    monkeypatch.setattr(engine, "device_count", no_device)
    monkeypatch.setattr(engine, "default_context", no_device)
    ans = Q.KernelStateAnsatz(n, 1, 1.0, Q.entanglement_graph(n, 1))
    with pytest.raises(ValueError, match=match):
        K.build_block_kernel_matrices(SingleComm(), ans, np.zeros((3, n)), truncation_error=1e-16, **kwargs)


def test_library_exports_the_entry_point(built):
    assert hasattr(engine.lib(), "qk_shot_block_sums_host")
