"""Strings of single-site operators and outcome marginals on the MI355X: qk_operator_strings_host (``Context.operator_expectations``,
``Context.marginals``) against the numpy mirror ``MPS.operator_expectation`` on identical tensors (1e-12) and dense state vectors,
the Pauli table against ``pauli_expectations`` (1e-13), full-support projector strings against ``amplitudes``, the outcomes of a
subset summing to 1, a window's Z marginals against the diagonal of ``window_rdms``, a ladder correlator against
``local_pair_paulis`` (the imaginary closing path), O^dagger = the complex conjugate, a doubled table entry (bit for bit), a
confusion-matrix mix, the bit guarantees (alone, with other strings, reordered, QK_OPSTR_BATCH = 1 / 3 / unset, run to run, norms,
the all-identity row), a NaN canary state, every rejection, and ``build_outcome_marginals`` on one rank against exact state
vectors (1e-10).  The tolerances are those of tests/test_gpu_pauli_strings.py.

The sets are small: chains of 1, 2, 6 and 12 sites.  The 12-site set has ragged bonds between its states and one general-gauge
state with a true bond of 70 (padded to 80: two 64-blocks with a ragged second block, and pad rows).

Measured on the MI355X: against the mirror max |dV| = 5.4e-16 and against dense vectors 3.7e-16 over the four chain lengths; the Pauli
table's real part equals ``pauli_expectations`` bit for bit on these states, max |Im| = 2.8e-16; projector strings against
|amplitude|^2 / <psi|psi> 3.4e-14 relative (p down to 1.2e-6); the 16 outcomes sum to 1 within 4.4e-16; window marginals against the
RDM diagonal 8.3e-17; the ladder correlator 2.7e-16; O^dagger against the conjugate 2.0e-16; the confusion mix 8.3e-17;
``build_outcome_marginals`` against exact state vectors 1.7e-15.  The file runs in 3 s."""
import functools
import itertools

import numpy as np
import pytest

import qml_cutensornet_amd as Q
from helpers import canary_copy, scrambled
from oracle import restatement as R
from qml_cutensornet_amd import engine
from test_op_strings_host import case_codes, operator_strings_from_dense
from test_pauli_strings_host import sparse_strings
from test_projected_host import dense

pytestmark = pytest.mark.gpu
N = 12
PAULI_TABLE = np.stack([engine.LOCAL_OPS[c] for c in "XYZ"])


def random_table(rng, n_ops=5):
    """Distinct random complex operators of spectral norm <= 1 (so every entry has magnitude <= 1 and every value too)."""
    t = rng.uniform(-1, 1, size=(n_ops, 2, 2)) + 1j * rng.uniform(-1, 1, size=(n_ops, 2, 2))
    return np.ascontiguousarray(t / np.maximum(1.0, np.linalg.norm(t, ord=2, axis=(1, 2)))[:, None, None])


@functools.lru_cache(maxsize=None)
def ragged_set():
    """Four 12-site states with ragged bonds between them: a general-gauge state with a true bond of 70 (a 64-bond chain grown by
    6 on every bond), a right-orthonormal chain capped at 5, a general-gauge chain capped at 20 and scaled by 3.7, and a
    right-orthonormal chain with the full profile up to 64."""
    rng = np.random.default_rng(70)
    prof = [min(2 ** min(k, N - k), 64) for k in range(N + 1)]
    big = scrambled(Q.random_mps(N, prof, rng), rng, grow=6)
    assert big.max_bond() == 70
    small = Q.random_mps(N, [min(c, 5) for c in prof], rng)
    mid = scrambled(Q.random_mps(N, [min(c, 20) for c in prof], rng), rng, scale=3.7)
    return (big, small, mid, Q.random_mps(N, prof, rng))


@functools.lru_cache(maxsize=None)
def short_sets():
    """Chains of 1, 2 and 6 sites, three states each, the last one in a general gauge where it has a bond."""
    rng = np.random.default_rng(71)
    out = {}
    for prof in ([1, 1], [1, 2, 1], [1, 2, 4, 8, 4, 2, 1]):
        n = len(prof) - 1
        ms = [Q.random_mps(n, prof, rng) for _ in range(3)]
        if n > 1:
            ms[2] = scrambled(ms[2], rng, scale=0.6)
        out[n] = tuple(ms)
    return out


@functools.lru_cache(maxsize=None)
def dense_of(key):
    states = ragged_set() if key == N else short_sets()[key]
    return tuple(dense(m) for m in states)


def states_of(n):
    return list(ragged_set() if n == N else short_sets()[n])


def run(ctx, states, codes, table, norms=False):
    with ctx.upload(states) as s:
        return ctx.operator_expectations(s, codes, ops=table, norms=norms)


# ---- 1. against the numpy mirror and dense vectors ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 6, N])
def test_against_the_mirror_and_dense_vectors(gpu_ctx, n):
    rng = np.random.default_rng(100 + n)
    states = states_of(n)
    table = random_table(rng)
    codes = case_codes(n, rng, len(table))
    if n == N:  # supports of 9, 10 and 11 sites beside the full one of case_codes
        longer = np.zeros((3, n), dtype=np.uint8)
        for row, (a, b) in zip(longer, ((0, 8), (2, 11), (1, 11))):
            row[a : b + 1] = rng.integers(1, len(table) + 1, size=b + 1 - a)
        codes = np.ascontiguousarray(np.vstack([longer, codes]))
    V, nrm = run(gpu_ctx, states, codes, table, norms=True)
    assert V.shape == (len(states), len(codes)) and V.dtype == np.complex128
    mirror = np.stack([m.operator_expectation(table, codes) for m in states])
    exact = np.stack([operator_strings_from_dense(psi, n, table, codes) for psi in dense_of(n)])
    e_m, e_d = float(np.abs(V - mirror).max()), float(np.abs(V - exact).max())
    share = float((np.abs(mirror) >= 1e-3).mean())
    print(f"operator strings, {n} sites: {len(states)} states x {len(codes)} strings, max |dV| = {e_m:.3e} (mirror), {e_d:.3e} (dense); "
          f"max |V| = {np.abs(V).max():.3f}, max |Im V| = {np.abs(V.imag).max():.3f}, share of |V| >= 1e-3: {share:.2f}")
    assert share >= 0.5 and np.abs(V.imag).max() > 1e-3 and np.abs(V).max() <= 1.0 + 1e-12
    assert e_m < 1e-12 and e_d < 1e-12
    for m, psi, got in zip(states, dense_of(n), nrm):
        want = float(np.vdot(psi, psi).real)
        assert abs(got - want) < 1e-12 * want
    ident = np.flatnonzero(~codes.any(axis=1))
    assert ident.size and np.all(V[:, ident] == 1.0 + 0.0j)
    assert np.array_equal(V[:, -1], V[:, 3 if n == N else 0])  # the duplicate of case_codes' first row


# ---- 2. the Pauli table through the new entry ------------------------------------------------------------------------------
def test_pauli_table_against_pauli_expectations(gpu_ctx):
    rng = np.random.default_rng(2)
    S = np.vstack([sparse_strings(N, 40, rng), rng.integers(0, 4, size=(4, N)).astype(np.uint8), np.zeros((1, N), dtype=np.uint8)])
    with gpu_ctx.upload(states_of(N)) as s:
        P, pn = gpu_ctx.pauli_expectations(s, S, norms=True)
        V, vn = gpu_ctx.operator_expectations(s, S, ops=PAULI_TABLE, norms=True)
    d_re, d_im = float(np.abs(V.real - P).max()), float(np.abs(V.imag).max())
    print(f"Pauli table through operator strings: max |Re - pauli_expectations| = {d_re:.3e}, max |Im| = {d_im:.3e}")
    assert (np.abs(P) >= 1e-3).mean() >= 0.5
    assert d_re < 1e-13 and d_im < 1e-13
    assert np.array_equal(vn, pn)


# ---- 3. full-support projector strings against amplitudes --------------------------------------------------------------------
@pytest.mark.parametrize("n", [6, N])
def test_full_support_projectors_against_amplitudes(gpu_ctx, n):
    rng = np.random.default_rng(3)
    bases = np.vstack([engine.random_bases(9, n, 5), np.full((1, n), 3), np.full((1, n), 1), np.full((1, n), 2)]).astype(np.uint8)
    bits = rng.integers(0, 2, size=bases.shape).astype(np.uint8)
    with gpu_ctx.upload(states_of(n)) as s:
        amp, nrm = gpu_ctx.amplitudes(s, bits, bases=bases, norms=True)
        p = gpu_ctx.marginals(s, bits, bases)
    want = np.abs(amp) ** 2 / nrm[:, None]
    rel = float((np.abs(p - want) / want).max())
    print(f"full-support projector strings vs |amplitude|^2 / <psi|psi>, {n} sites: max relative difference {rel:.3e} (p from {want.min():.2e} to {want.max():.2e})")
    assert p.dtype == np.float64 and p.shape == want.shape and rel < 1e-12


# ---- 4. the outcomes of a subset sum to 1 ------------------------------------------------------------------------------------
def test_outcomes_of_a_subset_sum_to_one(gpu_ctx):
    sub, basis = (1, 4, 5, 10), (1, 3, 2, 2)  # non-contiguous, mixed bases
    bases = np.zeros(N, dtype=np.uint8)
    bases[list(sub)] = basis
    bits = np.ones((16, N), dtype=np.uint8)  # the bits of the unmeasured qubits are ignored
    bits[:, list(sub)] = list(itertools.product((0, 1), repeat=4))
    with gpu_ctx.upload(states_of(N)) as s:
        p = gpu_ctx.marginals(s, bits, bases)
    tot = p.sum(axis=1)
    print(f"16 outcomes of qubits {sub} in bases {basis}: max |sum - 1| = {np.abs(tot - 1).max():.3e}, min p = {p.min():.3e}")
    assert np.abs(tot - 1.0).max() < 1e-12 and p.min() > -1e-12
    mirror = np.stack([m.marginal(bits, bases) for m in states_of(N)])
    assert np.abs(p - mirror).max() < 1e-12


# ---- 5. Z marginals of a window are the diagonal of its RDM --------------------------------------------------------------------
def test_window_marginals_are_the_rdm_diagonal(gpu_ctx):
    w = 3
    starts = [0, 4, N - w]
    bits = np.zeros((8 * len(starts), N), dtype=np.uint8)
    bases = np.zeros_like(bits)
    for j, a in enumerate(starts):
        bits[8 * j : 8 * j + 8, a : a + w] = list(itertools.product((0, 1), repeat=w))
        bases[8 * j : 8 * j + 8, a : a + w] = 3
    with gpu_ctx.upload(states_of(N)) as s:
        p = gpu_ctx.marginals(s, bits, bases)
        rho = gpu_ctx.window_rdms(s, w, starts=starts)
    diag = np.diagonal(rho, axis1=2, axis2=3).real.reshape(len(rho), -1)
    err = float(np.abs(p - diag).max())
    print(f"Z marginals of 3-qubit windows at {starts} vs diag window_rdms: max |d| = {err:.3e}")
    assert err < 1e-12


# ---- 6. a ladder correlator: the imaginary closing path ------------------------------------------------------------------------
def test_ladder_correlator_against_pair_paulis(gpu_ctx):
    D = 3
    pairs = engine.pair_table(N, D)
    specs = [(("01", "10"), (int(a), int(b))) for a, b in pairs]
    with gpu_ctx.upload(states_of(N)) as s:
        T = gpu_ctx.local_pair_paulis(s, max_dist=D)
        V = gpu_ctx.operator_expectations(s, specs)
    want = (T[:, :, 1, 1] + T[:, :, 2, 2] + 1j * (T[:, :, 2, 1] - T[:, :, 1, 2])) / 4
    err = float(np.abs(V - want).max())
    print(f"<|0><1|_a |1><0|_b> vs local_pair_paulis(max_dist={D}): max |d| = {err:.3e}, max |Im| = {np.abs(want.imag).max():.3e}")
    assert np.abs(want.imag).max() > 1e-3  # the imaginary part is really there
    assert err < 1e-12


# ---- 7. - 9. adjoint, a doubled entry, a confusion matrix --------------------------------------------------------------------------
def test_adjoint_doubling_and_confusion_mix(gpu_ctx):
    rng = np.random.default_rng(7)
    table = random_table(rng) / 2  # the doubled operator keeps its entries <= 1
    codes = case_codes(N, rng, len(table))
    eps0, eps1 = 0.03, 0.08
    proj = np.stack([engine.LOCAL_OPS["0"], engine.LOCAL_OPS["1"], engine.LOCAL_OPS["R"], (1 - eps0) * engine.LOCAL_OPS["0"] + eps1 * engine.LOCAL_OPS["1"]])
    rows = np.zeros((3, N), dtype=np.uint8)
    rows[:, 2], rows[:, 9] = 3, 2
    rows[:, 6] = (4, 1, 2)  # the mix, then its two projectors, between two measured qubits
    doubled = table.copy()
    doubled[2] *= 2
    with gpu_ctx.upload(states_of(N)) as s:
        V = gpu_ctx.operator_expectations(s, codes, ops=table)
        Vd = gpu_ctx.operator_expectations(s, codes, ops=np.ascontiguousarray(table.conj().transpose(0, 2, 1)))
        V2 = gpu_ctx.operator_expectations(s, codes, ops=doubled)
        mix = gpu_ctx.operator_expectations(s, rows, ops=proj)
    e_adj = float(np.abs(Vd - V.conj()).max())
    uses = (codes == 3).sum(axis=1)
    assert (uses == 1).any() and (uses == 0).any() and (uses >= 2).any()
    e_mix = float(np.abs(mix[:, 0] - ((1 - eps0) * mix[:, 1] + eps1 * mix[:, 2])).max())
    print(f"O^dagger vs conj: max |d| = {e_adj:.3e}; confusion mix vs mix of marginals: {e_mix:.3e}; strings using the doubled operator 0 / 1 / 2+ times: "
          f"{int((uses == 0).sum())} / {int((uses == 1).sum())} / {int((uses >= 2).sum())}")
    assert e_adj < 1e-13 and e_mix < 1e-13
    assert np.array_equal(V2, V * (2.0 ** uses)[None, :])  # 2 O at one code: a power of two per use, bit for bit; the others keep their bits
    assert np.abs(V[:, uses >= 1]).max() > 1e-3


# ---- 10. bit guarantees ----------------------------------------------------------------------------------------------------------
def test_bit_guarantees(gpu_ctx, monkeypatch):
    rng = np.random.default_rng(10)
    table = random_table(rng)
    codes = case_codes(N, rng, len(table), count=12)
    states = states_of(N)
    monkeypatch.delenv("QK_OPSTR_BATCH", raising=False)
    alone = run(gpu_ctx, [states[0]], codes, table)
    with gpu_ctx.upload(states) as s:
        V1, nrm = gpu_ctx.operator_expectations(s, codes, ops=table, norms=True)
        V2 = gpu_ctx.operator_expectations(s, codes, ops=table)
        Vr = gpu_ctx.operator_expectations(s, codes[::-1], ops=table)
        one = gpu_ctx.operator_expectations(s, codes[5:6], ops=table)
        bigger = np.vstack([table, random_table(rng, 3)])  # other operators in the table, other strings in the call
        Vb = gpu_ctx.operator_expectations(s, np.vstack([case_codes(N, rng, len(bigger), count=5), codes]), ops=bigger)
        batched = []
        for cap in ("1", "3"):
            monkeypatch.setenv("QK_OPSTR_BATCH", cap)
            batched.append(gpu_ctx.operator_expectations(s, codes, ops=table))
        monkeypatch.setenv("QK_OPSTR_BATCH", "0")  # read per call: a bad value is an error of that call
        with pytest.raises(engine.QkError, match="QK_OPSTR_BATCH"):
            gpu_ctx.operator_expectations(s, codes, ops=table)
        monkeypatch.delenv("QK_OPSTR_BATCH")
        V3 = gpu_ctx.operator_expectations(s, codes, ops=table)
        F, ln = gpu_ctx.local_paulis(s, norms=True)
    assert np.array_equal(alone[0], V1[0])
    assert np.array_equal(V1, V2) and np.array_equal(V1, V3)
    assert np.array_equal(Vr, V1[:, ::-1])
    assert np.array_equal(one[:, 0], V1[:, 5])
    assert np.array_equal(Vb[:, -len(codes):], V1)
    for Vc in batched:
        assert np.array_equal(Vc, V1)
    assert np.array_equal(nrm, ln)
    ident = np.flatnonzero(~codes.any(axis=1))
    assert ident.size and np.all(V1[:, ident] == 1.0 + 0.0j)


# ---- 11. a NaN canary state ------------------------------------------------------------------------------------------------------
def test_a_canary_state_spoils_its_own_row_only(gpu_ctx, monkeypatch):
    rng = np.random.default_rng(11)
    table = random_table(rng)
    codes = case_codes(N, rng, len(table), count=12)
    states = states_of(N)
    ident = ~codes.any(axis=1)
    monkeypatch.delenv("QK_OPSTR_BATCH", raising=False)
    with gpu_ctx.upload(states) as dc:
        clean, cn = gpu_ctx.operator_expectations(dc, codes, ops=table, norms=True)
        for idx in (0, 2):  # the bond-70 state; a state between two clean ones
            dirty = [canary_copy(m) if i == idx else m for i, m in enumerate(states)]
            with gpu_ctx.upload(dirty) as dd:
                for cap in (None, "1"):
                    if cap:
                        monkeypatch.setenv("QK_OPSTR_BATCH", cap)
                    got, gn = gpu_ctx.operator_expectations(dd, codes, ops=table, norms=True)
                    monkeypatch.delenv("QK_OPSTR_BATCH", raising=False)
                    rows = np.arange(len(states)) != idx
                    assert np.array_equal(got[rows], clean[rows]) and np.array_equal(gn[rows], cn[rows])
                    assert np.isnan(got[idx, ~ident].real).all() and np.isnan(got[idx, ~ident].imag).all() and np.isnan(gn[idx])
                    assert np.all(got[idx, ident] == 1.0 + 0.0j)  # written without arithmetic
            again = gpu_ctx.operator_expectations(dc, codes, ops=table)
            assert np.array_equal(again, clean)
    assert np.isfinite(clean.real).all() and np.isfinite(clean.imag).all()


# ---- 12. rejections ---------------------------------------------------------------------------------------------------------------
def test_rejections(gpu_ctx, monkeypatch):
    rng = np.random.default_rng(0)
    L = engine.lib()
    call = L.qk_operator_strings_host
    out = np.zeros((2, 2, 2))
    S = np.array([[0, 3, 1, 0], [2, 0, 0, 0]], dtype=np.uint8)
    ops = np.ascontiguousarray(PAULI_TABLE).view(np.float64).reshape(3, 2, 2, 2).copy()  # [code - 1][s'][s][re, im]
    monkeypatch.delenv("QK_OPSTR_BATCH", raising=False)
    states = [Q.random_mps(4, [1, 2, 4, 2, 1], rng) for _ in range(2)]
    with gpu_ctx.upload(states) as s, s.to_f32() as s32:
        h, sh, o, st, ou = gpu_ctx._h, s.handle, ops.ctypes.data, S.ctypes.data, out.ctypes.data

        def rejected(match, *args):
            rc = call(*args)
            assert rc == -1, (match, rc)  # QK_EINVAL
            with pytest.raises(engine.QkError, match=match):
                engine._check(rc, "opstr")

        for args, name in (((None, sh, 3, o, 2, st, ou, None), "ctx"), ((h, None, 3, o, 2, st, ou, None), "set"), ((h, sh, 3, None, 2, st, ou, None), "ops"),
                           ((h, sh, 3, o, 2, None, ou, None), "strings"), ((h, sh, 3, o, 2, st, None, None), "out")):
            rejected(f"{name} is null", *args)
        rejected("complex64", h, s32.handle, 3, o, 2, st, ou, None)
        with engine.Context(0) as other:
            rejected("another context", other._h, sh, 3, o, 2, st, ou, None)
        rejected(r"n_strings must be >= 1 \(got 0\)", h, sh, 3, o, 0, st, ou, None)
        rejected(r"n_ops must be in 1 \.\. 255 \(got 0\)", h, sh, 0, o, 2, st, ou, None)
        rejected(r"n_ops must be in 1 \.\. 255 \(got 256\)", h, sh, 256, o, 2, st, ou, None)
        for bad_value, part in ((float("nan"), "real"), (float("inf"), "imaginary")):
            bad = ops.copy()
            bad[1, 1, 0, 0 if part == "real" else 1] = bad_value
            rejected(rf"ops\[1\]\[1\]\[0\] \(code 2\) has a {part} part that is not finite", h, sh, 3, bad.ctypes.data, 2, st, ou, None)
        badS = S.copy()
        badS[1, 2] = 4
        rejected(r"strings\[1\]\[2\] = 4 is above n_ops = 3", h, sh, 3, o, 2, badS.ctypes.data, ou, None)
        rejected(r"strings\[0\]\[1\] = 3 is above n_ops = 2", h, sh, 2, o, 2, st, ou, None)
        monkeypatch.setenv("QK_OPSTR_BATCH", "-2")
        rejected(r"QK_OPSTR_BATCH must be >= 1 \(got \"-2\"\)", h, sh, 3, o, 2, st, ou, None)
        monkeypatch.delenv("QK_OPSTR_BATCH")
        # the Python layer names a bad spec and a bad table before the library is called
        with pytest.raises(ValueError, match="0Q"):
            gpu_ctx.operator_expectations(s, [("0Q", (1, 2))])
        with pytest.raises(ValueError, match="bases"):
            gpu_ctx.marginals(s, np.zeros((1, 4), dtype=int), [3, 4, 0, 0])
        # the context works afterwards; norms may be NULL
        engine._check(call(h, sh, 3, o, 2, st, ou, None), "opstr")
        want = np.stack([m.operator_expectation(PAULI_TABLE, S) for m in states])
        assert np.abs(out[..., 0] + 1j * out[..., 1] - want).max() < 1e-12
    # a state of norm 0 is QK_EDEVICE and is named
    zero = Q.MPS([t * 0 for t in states[1].tensors])
    with gpu_ctx.upload([states[0], zero]) as s:
        with pytest.raises(engine.QkError, match="error -2: qk_operator_strings_host: state 1 has norm 0"):  # QK_EDEVICE
            gpu_ctx.operator_expectations(s, S, ops=PAULI_TABLE)
    with gpu_ctx.upload(states) as s:
        assert np.abs(gpu_ctx.operator_expectations(s, S, ops=PAULI_TABLE) - want).max() < 1e-12


# ---- 13. build_outcome_marginals -----------------------------------------------------------------------------------------------
def test_build_outcome_marginals_against_exact_state_vectors(gpu_ctx):
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_outcome_marginals

    n = 8
    rng = np.random.default_rng(13)
    ans = Q.KernelStateAnsatz(n, 2, 1.0, Q.entanglement_graph(n, 2))
    X = R.synthetic_features(5, n, 31)
    bases = np.where(rng.random((20, n)) < 0.5, rng.integers(1, 4, size=(20, n)), 0).astype(np.uint8)
    bases[0] = 0      # no measured qubit
    bases[1] = 3      # every qubit, Z
    bits = rng.integers(0, 2, size=(20, n)).astype(np.uint8)
    p = build_outcome_marginals(SingleComm(), ans, X, bits, bases, truncation_error=1e-16)
    table, codes = engine.marginal_strings(bits, bases, n)
    exact = []
    for x in X:
        circ = ans.circuit_for_data(x)
        psi = R.statevector(n, [(name, tuple(qs), (q[0] if q else None)) for name, qs, q in circ.as_tuples()])
        exact.append(operator_strings_from_dense(psi, n, table, codes).real)
    err = float(np.abs(p - np.stack(exact)).max())
    print(f"build_outcome_marginals, one rank, {n} qubits: max |p - exact| = {err:.3e}, p from {p.min():.2e} to {p.max():.2e}")
    assert p.shape == (5, 20) and p.dtype == np.float64 and err < 1e-10
    assert np.all(p[:, 0] == 1.0)
    shared = build_outcome_marginals(SingleComm(), ans, X, bits[:3], bases[2], truncation_error=1e-16)  # one shared row of bases
    assert shared.shape == (5, 3) and np.array_equal(shared[:, 2], build_outcome_marginals(SingleComm(), ans, X, bits[2:3], bases[2], truncation_error=1e-16)[:, 0])
