"""MPO observables on the MI355X: qk_mpo_expectations_host (``Context.mpo_expectations``) against the numpy mirror
``MPS.mpo_expectation`` on the general-gauge twins of ``helpers.gauge_sets`` (20 sites, bonds to 128) and of ``helpers.gauge_set_300``
(18 sites, bonds to 300: several 64 x 64 blocks, ragged last blocks, five planes stacked to M = 1520), term-built MPOs against the
sum of their terms through ``operator_expectations`` on the device, twins against originals, the bit guarantees (a bond-1 MPO
against its operator string, alone against in a list, a reversed list, QK_MPO_BATCH = 1 against unset, one tensor scaled by 2,
explicit zero blocks, the all-identity MPO), a NaN canary state, every rejection, and the two drivers.

The tolerance of a value is 1e-12 S (1e-11 S between twins and originals): the project's 1e-12 for unit-scale strings times the
operator bound S >= ||H|| that tests/test_mpo_host.py restates -- sum_t |c_t| prod ||O||_2 for a term-built MPO, S_H^2 for H @ H, 1 for
the random dense MPOs, whose matricised tensors have spectral norm 1."""
import functools

import numpy as np
import pytest

import qml_cutensornet_amd as Q
from helpers import canary_copy, gauge_set_300, gauge_sets
from oracle import restatement as R
from qml_cutensornet_amd import engine
from test_mpo_host import LADDER, exponential_terms, hamming_terms, heisenberg_terms, random_dense_mpo, term_bound

pytestmark = pytest.mark.gpu
N = 20
DENSE_BONDS = ([1, 3, 5, 2, 4, 6, 3, 1, 2, 5, 7, 4, 2, 3, 6, 8, 5, 3, 2, 2, 1], [1, 2, 4, 8, 16, 32, 16, 8, 4, 3, 2, 2, 3, 4, 2, 2, 3, 2, 2, 2, 1])


@functools.lru_cache(maxsize=None)
def cases20():
    """name -> (Mpo, S, terms or None) on 20 sites."""
    rng = np.random.default_rng(200)
    heis, expo, ham = heisenberg_terms(N), exponential_terms(N, "Z", "Z", 1.0, 0.7), hamming_terms((2, 5, 9, 13, 17), 3)
    win = heisenberg_terms(N, sites=range(7, 13))
    Hw = engine.mpo_from_terms(N, win)
    out = {
        "heisenberg": (engine.mpo_from_terms(N, heis), term_bound(heis), heis),
        "exponential": (engine.mpo_exponential(N, "Z", "Z", 1.0, 0.7), term_bound(expo), expo),
        "hamming": (engine.mpo_from_terms(N, ham), term_bound(ham), ham),
        "squared": (Hw @ Hw, term_bound(win) ** 2, None),
        "dense A": (random_dense_mpo(rng, DENSE_BONDS[0]), 1.0, None),
        "dense B": (random_dense_mpo(rng, DENSE_BONDS[1]), 1.0, None),
    }
    assert out["squared"][0].max_bond() == 25 and out["hamming"][0].max_bond() == 10 and out["dense B"][0].max_bond() == 32
    assert out["heisenberg"][0].max_bond() == 5 and out["exponential"][0].max_bond() == 3
    return out


def run(ctx, states, mpos, norms=False):
    with ctx.upload(list(states)) as s:
        return ctx.mpo_expectations(s, mpos, norms=norms)


def term_sum(ctx, s, terms, ops=None):
    V = ctx.operator_expectations(s, [(names, qubits) for _, names, qubits in terms], ops=ops)
    return V @ np.array([c for c, _, _ in terms], dtype=np.complex128)


# ---- 1. the 20-site twins: mirror, term sums, originals --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["heisenberg", "exponential", "hamming", "squared", "dense A", "dense B"])
def test_twins_against_the_mirror_the_term_sum_and_the_originals(gpu_ctx, name):
    H, S, terms = cases20()[name]
    originals, twins = gauge_sets()
    with gpu_ctx.upload(list(twins)) as s:
        V = gpu_ctx.mpo_expectations(s, [H])
        T = term_sum(gpu_ctx, s, terms) if terms is not None else None
    Vo = run(gpu_ctx, originals, [H])
    assert V.shape == (6, 1) and V.dtype == np.complex128
    mirror = np.array([m.mpo_expectation(H) for m in twins])
    e_m, e_o = float(np.abs(V[:, 0] - mirror).max()), float(np.abs(V - Vo).max())
    e_t = float(np.abs(V[:, 0] - T).max()) if T is not None else float("nan")
    print(f"MPO {name}: bond {H.max_bond()}, S = {S:.4g}, max |V| = {np.abs(V).max():.3e}; max |d| / S = {e_m / S:.3e} (mirror), {e_t / S:.3e} (term sum), "
          f"{e_o / S:.3e} (twins vs originals)")
    assert np.abs(V).max() <= S * (1 + 1e-12) and np.abs(V).max() > 0
    assert e_m < 1e-12 * S
    if T is not None:
        assert e_t < 1e-12 * S
    assert e_o < 1e-11 * S


# ---- 2. bonds to 300: stacked planes over several blocks, a support inside the chain ----------------------------------------
def test_bonds_to_300_against_the_mirror(gpu_ctx):
    n = 18
    twins = gauge_set_300()[1]
    full_t = heisenberg_terms(n)
    inner_t = [(0.9, "ZZ", (a, a + 1)) for a in range(7, 11)] + [(0.4, "X", (7,)), (-0.3, "Y", (11,))]
    full, inner = engine.mpo_from_terms(n, full_t), engine.mpo_from_terms(n, inner_t)
    assert full.max_bond() == 5 and inner.max_bond() == 3 and list(inner.bonds[:8]) == [1] * 8 and list(inner.bonds[12:]) == [1] * 7
    V, nrm = run(gpu_ctx, twins, [full, inner], norms=True)
    with gpu_ctx.upload(list(twins)) as s:
        ln = gpu_ctx.local_paulis(s, norms=True)[1]
    assert np.array_equal(nrm, ln)
    for j, (H, S) in enumerate(((full, term_bound(full_t)), (inner, term_bound(inner_t)))):
        mirror = np.array([m.mpo_expectation(H) for m in twins])
        err = float(np.abs(V[:, j] - mirror).max())
        print(f"bonds to 300, MPO bond {H.max_bond()}: S = {S:.4g}, max |V| = {np.abs(V[:, j]).max():.3e}, max |d| / S = {err / S:.3e}")
        assert np.abs(V[:, j]).max() > 1e-3 and err < 1e-12 * S


# ---- 3. bit guarantees ----------------------------------------------------------------------------------------------------------
def test_bit_guarantees(gpu_ctx, monkeypatch):
    rng = np.random.default_rng(3)
    twins = list(gauge_sets()[1])
    named = [cases20()[k][0] for k in ("heisenberg", "dense A", "exponential", "hamming")]
    monkeypatch.delenv("QK_MPO_BATCH", raising=False)
    # a bond-1 MPO against its operator string: ladder operators, gaps, the ends, a single site
    specs = [(("Sp", "Sm"), (3, 11)), (("G", "X", "Sm"), (0, 7, 19)), (("Y",), (9,)), (("Z", "G", "0", "R"), (12, 13, 14, 16)), (("G",) * N, tuple(range(N)))]
    table, codes = engine.operator_strings(N, specs, LADDER)
    products = [engine.mpo_product(N, table, row) for row in codes]
    ident = engine.Mpo([np.eye(2).reshape(1, 1, 2, 2)] * N)
    # explicit zero blocks: a dense MPO with blocks set to zero, some as -0.0
    zt = [t.copy() for t in random_dense_mpo(rng, [1, 3, 4, 3] + [2] * (N - 4) + [1]).tensors]
    zt[1][0, 1], zt[1][2, 1], zt[2][1, 2], zt[2][3, 0] = 0.0, 0.0, 0.0, -0.0
    zt[2][:, 1] = 0.0  # a v without a block: a zero plane
    zt[5][1, 0] = 0.0
    zeros = engine.Mpo(zt)
    doubled = engine.Mpo([t * 2 if k == 6 else t for k, t in enumerate(named[1].tensors)])
    with gpu_ctx.upload(twins) as s:
        ops = gpu_ctx.operator_expectations(s, codes, ops=table)
        Vp, pn = gpu_ctx.mpo_expectations(s, products, norms=True)
        everything = named + [zeros, ident, doubled]
        V1, nrm = gpu_ctx.mpo_expectations(s, everything, norms=True)
        V2 = gpu_ctx.mpo_expectations(s, everything)
        Vr = gpu_ctx.mpo_expectations(s, everything[::-1])
        singles = [gpu_ctx.mpo_expectations(s, [H])[:, 0] for H in everything]
        Vz = gpu_ctx.mpo_expectations(s, [zeros, named[0]])  # the same list in another order
        monkeypatch.setenv("QK_MPO_BATCH", "1")
        Vb = gpu_ctx.mpo_expectations(s, everything)
        monkeypatch.setenv("QK_MPO_BATCH", "0")  # read per call: a bad value is an error of that call
        with pytest.raises(engine.QkError, match=r"QK_MPO_BATCH must be >= 1 \(got \"0\"\)"):
            gpu_ctx.mpo_expectations(s, everything)
        monkeypatch.delenv("QK_MPO_BATCH")
        V3 = gpu_ctx.mpo_expectations(s, everything)
        ln = gpu_ctx.local_paulis(s, norms=True)[1]
    alone = run(gpu_ctx, [twins[3]], everything)
    assert np.array_equal(Vp, ops) and np.abs(ops).max() > 1e-3 and np.abs(ops.imag).max() > 1e-4
    assert np.array_equal(V1, V2) and np.array_equal(V1, V3) and np.array_equal(V1, Vb)
    assert np.array_equal(Vr, V1[:, ::-1])
    for j, v in enumerate(singles):
        assert np.array_equal(v, V1[:, j])
    assert np.array_equal(alone[0], V1[3])
    assert np.array_equal(Vz[:, 0], V1[:, 4]) and np.array_equal(Vz[:, 1], V1[:, 0])
    assert np.array_equal(V1[:, 6], 2 * V1[:, 1]) and np.abs(V1[:, 1]).max() > 0
    assert np.all(V1[:, 5] == 1.0 + 0.0j)
    assert np.array_equal(nrm, ln) and np.array_equal(pn, ln)
    mirror = np.array([m.mpo_expectation(zeros) for m in twins])
    assert np.abs(V1[:, 4] - mirror).max() < 1e-12 and np.abs(mirror).max() > 0


# ---- 4. a NaN canary state ------------------------------------------------------------------------------------------------------
def test_a_canary_state_spoils_its_own_row_only(gpu_ctx, monkeypatch):
    twins = list(gauge_sets()[1])
    mpos = [cases20()[k][0] for k in ("heisenberg", "dense A", "hamming")] + [engine.Mpo([np.eye(2).reshape(1, 1, 2, 2)] * N)]
    monkeypatch.delenv("QK_MPO_BATCH", raising=False)
    idx = 3  # the profile that reaches bond 128, between clean states
    dirty = [canary_copy(m) if i == idx else m for i, m in enumerate(twins)]
    rows = np.arange(len(twins)) != idx
    with gpu_ctx.upload(twins) as dc:
        clean, cn = gpu_ctx.mpo_expectations(dc, mpos, norms=True)
        with gpu_ctx.upload(dirty) as dd:
            got, gn = gpu_ctx.mpo_expectations(dd, mpos, norms=True)
        again = gpu_ctx.mpo_expectations(dc, mpos)
    assert np.isfinite(clean.real).all() and np.isfinite(clean.imag).all()
    assert np.array_equal(got[rows], clean[rows]) and np.array_equal(gn[rows], cn[rows])
    assert np.isnan(got[idx, :3].real).all() and np.isnan(got[idx, :3].imag).all() and np.isnan(gn[idx])
    assert got[idx, 3] == 1.0 + 0.0j  # written without arithmetic
    assert np.array_equal(again, clean)


# ---- 5. rejections ---------------------------------------------------------------------------------------------------------------
def test_rejections(gpu_ctx, monkeypatch):
    rng = np.random.default_rng(0)
    call = engine.lib().qk_mpo_expectations_host
    n = 4
    H = engine.mpo_from_terms(n, heisenberg_terms(n))
    P = engine.mpo_product(n, "XZ", (1, 2))
    bonds = np.ascontiguousarray(np.stack([H.bonds, P.bonds]), dtype=np.int32)
    tens = np.ascontiguousarray(np.concatenate([H.packed(), P.packed()]))
    out = np.zeros((2, 2, 2))
    monkeypatch.delenv("QK_MPO_BATCH", raising=False)
    states = [Q.random_mps(n, [1, 2, 4, 2, 1], rng) for _ in range(2)]
    with gpu_ctx.upload(states) as s, s.to_f32() as s32:
        h, sh, b, t, ou = gpu_ctx._h, s.handle, bonds.ctypes.data, tens.ctypes.data, out.ctypes.data

        def rejected(match, *args):
            rc = call(*args)
            assert rc == -1, (match, rc)  # QK_EINVAL
            with pytest.raises(engine.QkError, match=match):
                engine._check(rc, "mpo")

        for args, name in (((None, sh, 2, b, t, ou, None), "ctx"), ((h, None, 2, b, t, ou, None), "set"), ((h, sh, 2, None, t, ou, None), "bonds"),
                           ((h, sh, 2, b, None, ou, None), "tensors"), ((h, sh, 2, b, t, None, None), "out")):
            rejected(f"{name} is null", *args)
        rejected("complex64", h, s32.handle, 2, b, t, ou, None)
        with engine.Context(0) as other:
            rejected("another context", other._h, sh, 2, b, t, ou, None)
        rejected(r"n_mpos must be >= 1 \(got 0\)", h, sh, 0, b, t, ou, None)
        for m, k, w in ((0, 2, 33), (1, 3, 0), (1, 1, -4)):
            bad = bonds.copy()
            bad[m, k] = w
            rejected(rf"bonds\[{m}\]\[{k}\] = {w} is outside 1 \.\. 32 \(MPO {m}, cut {k}\)", h, sh, 2, bad.ctypes.data, t, ou, None)
        for m, k in ((1, 0), (0, n)):
            bad = bonds.copy()
            bad[m, k] = 2
            rejected(rf"bonds\[{m}\]\[{k}\] = 2 must be 1", h, sh, 2, bad.ctypes.data, t, ou, None)
        # MPO 0, site 1 is [5][5][2][2]: entry [1][3][1][0]; MPO 1, site 2 is [1][1][2][2]: entry [0][0][0][1]
        at0 = 8 * int(H.bonds[0] * H.bonds[1]) + 8 * (1 * int(H.bonds[2]) + 3) + 2 * (2 * 1 + 0)
        at1 = len(H.packed()) + 8 * 2 + 2 * 1 + 1
        assert H.bonds[1] == 5 and H.bonds[2] == 5
        for at, value, where in ((at0, float("nan"), r"MPO 0, site 1: W\[1\]\[3\]\[1\]\[0\] has a real part"), (at1, float("inf"), r"MPO 1, site 2: W\[0\]\[0\]\[0\]\[1\] has a imaginary part")):
            bad = tens.copy()
            bad[at] = value
            rejected(where + " that is not finite", h, sh, 2, b, bad.ctypes.data, ou, None)
        monkeypatch.setenv("QK_MPO_BATCH", "-2")
        rejected(r"QK_MPO_BATCH must be >= 1 \(got \"-2\"\)", h, sh, 2, b, t, ou, None)
        monkeypatch.delenv("QK_MPO_BATCH")
        # the Python layer names a bad list before the library is called
        with pytest.raises(ValueError, match="Mpo 0 has 5 sites"):
            gpu_ctx.mpo_expectations(s, [engine.mpo_product(5, "X", (0,))])
        with pytest.raises(ValueError, match="single Mpo"):
            gpu_ctx.mpo_expectations(s, H)
        # the context works afterwards; norms may be NULL
        engine._check(call(h, sh, 2, b, t, ou, None), "mpo")
        want = np.array([[m.mpo_expectation(H), m.mpo_expectation(P)] for m in states])
        assert np.abs(out[..., 0] + 1j * out[..., 1] - want).max() < 1e-12 * term_bound(heisenberg_terms(n))
    # a state of norm 0 is QK_EDEVICE and is named
    zero = Q.MPS([t * 0 for t in states[1].tensors])
    with gpu_ctx.upload([states[0], zero]) as s:
        with pytest.raises(engine.QkError, match="error -2: qk_mpo_expectations_host: state 1 has norm 0"):  # QK_EDEVICE
            gpu_ctx.mpo_expectations(s, [H])
    with gpu_ctx.upload(states) as s:
        assert np.abs(gpu_ctx.mpo_expectations(s, [H, P]) - want).max() < 1e-12 * term_bound(heisenberg_terms(n))


# ---- 6. the drivers -----------------------------------------------------------------------------------------------------------
def test_drivers_against_the_mirror(gpu_ctx):
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_mpo_expectations, build_projected_kernel_matrix

    n = 8
    ans = Q.KernelStateAnsatz(n, 2, 1.0, Q.entanglement_graph(n, 2))
    X = R.synthetic_features(6, n, 31)
    heis, expo = heisenberg_terms(n), exponential_terms(n, "Z", "Z", 1.0, 0.7)
    mpos = [engine.mpo_from_terms(n, heis), engine.mpo_exponential(n, "Z", "Z", 1.0, 0.7), engine.mpo_from_terms(n, hamming_terms((0, 2, 3, 5, 7), 3))]
    bounds = np.array([term_bound(heis), term_bound(expo), 10.0])
    V = build_mpo_expectations(SingleComm(), ans, X, mpos, truncation_error=1e-16)
    states = [Q.simulate(ans.circuit_for_data(x), 1 - 1e-16) for x in X]
    mirror = np.array([[m.mpo_expectation(H) for H in mpos] for m in states])
    err = float((np.abs(V - mirror) / bounds).max())
    print(f"build_mpo_expectations, one rank, {n} qubits, 6 points: max |d| / S = {err:.3e}, max |V| = {np.abs(V).max():.3f}")
    assert V.shape == (6, 3) and V.dtype == np.complex128 and err < 1e-12
    K = build_projected_kernel_matrix(SingleComm(), ans, X, observables=mpos, truncation_error=1e-16)
    F = mirror.real
    want = np.exp(-(1.0 / 3) * ((F[None, :, :] - F[:, None, :]) ** 2).sum(axis=2))
    e_k = float(np.abs(K - want).max())
    print(f"build_projected_kernel_matrix(observables=[Mpo x 3]): max |K - mirror| = {e_k:.3e}, off-diagonal K from {K[~np.eye(6, dtype=bool)].min():.3e}")
    # |dK| <= g sum_m 2 |F_i - F_j| |d(F_i - F_j)| with |F_i - F_j| <= 2 S_m and |d(F_i - F_j)| <= 2e-12 S_m, and the rounding of exp
    assert K.shape == (6, 6) and e_k < (1.0 / 3) * (8e-12 * bounds**2).sum() + 1e-15
    assert np.array_equal(np.diag(K), np.ones(6))
