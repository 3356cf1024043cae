"""``Context.compress`` (qk_mps_set_compress) on the MI355X against the host mirror ``MPS.compress`` on the same tensors, its
identities, the downloaded tensors, gauge invariance, rank-deficient sets, the bit guarantees, the rejections, and
``build_capped_kernel_matrices`` with one and two ranks.

Shapes: the three 20-site profiles of tests/test_gpu_entanglement.py as ONE mixed set of six gauge-scrambled states (bonds 1, 2,
15/16/17: row padding; 47/48: the switch of the Jacobi path; 63/64/65 and 128: the GEMM blocks), every second state scaled by 3.7;
chains of 1, 2 and 3 sites; 600 six-site states (more states than resident workgroups).

The yardstick is the mirror, never the device's own output.  A comparison first asserts FROM THE MIRROR that the cut is well
defined -- the gap between the last kept and the first dropped weight is >= 1e-6 of the total at every bond a cap cuts, and for a
budget the dropped tail and the tail with one more value are both >= 1e-9 budget away from the threshold (the seeds below were
chosen on the CPU so that this holds) -- and then: equal bonds, |fidelity - mirror| and |discarded - mirror| <= 1e-12 (the spectra
tests' tolerance), infidelity between the device's and the mirror's state <= 1e-11 through ``ctx.overlaps`` (second order of a
subspace angle of at most 1e-15 / 1e-6, plus the rounding of 1 - x).

Measured on the MI355X (every test prints its figures): against the mirror, over the eight cases, |d fidelity| <= 1.8e-15, |d
discarded| <= 5.8e-14 (cap 1; 2.7e-15 otherwise) and infidelity device vs mirror <= 2.1e-15, at smallest gaps of 1.07e-6 (cap 48)
and 2.05e-6 (cap 16) and threshold distances of 4.6e-3 and 7.6e-2 of the budget; the identity holds to 2.2e-15, the norm to 2.6e-13
(through ``ctx.overlaps`` of the scrambled set); Gram without truncation 3.2e-13; golden states: isometries to 9.9e-15, amplitudes
vs mirror 2.4e-15."""
import functools
import os
import sys

import numpy as np
import pytest

import qml_cutensornet_amd as Q
from helpers import PROFILES, golden_mps_sets, scrambled
from oracle import restatement as R
from qml_cutensornet_amd import engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = {  # name: (max_bond, max_discard)
    "cap1": (1, 0.0), "cap8": (8, 0.0), "cap16": (16, 0.0), "cap17": (17, 0.0), "cap48": (48, 0.0), "cap200": (200, 0.0),
    "budget1e-3": (None, 1e-3), "budget1e-8": (None, 1e-8),
}
SEED = 135  # chosen on the CPU: every cut of every case below is well defined (assert_cut_well_defined)


def dense_state(tensors) -> np.ndarray:
    psi = np.asarray(tensors[0])
    for t in tensors[1:]:
        psi = np.tensordot(psi, t, axes=(psi.ndim - 1, 0))
    return psi.reshape(-1)


@functools.lru_cache(maxsize=None)
def mixed_states():
    rng = np.random.default_rng(SEED)
    return tuple(scrambled(Q.random_mps(20, PROFILES[k % 3], rng), rng, scale=3.7 if k % 2 else 1.0) for k in range(6))


@functools.lru_cache(maxsize=None)
def mirror(case):
    """The host mirror of a case on the mixed set, computed once: [(MPS, discarded, singular values per bond)]."""
    cap, budget = CASES[case]
    return tuple(m._compress(cap, budget, 1e-16) for m in mixed_states())


@functools.lru_cache(maxsize=None)
def original_spectra():
    return tuple(m.bond_spectra() for m in mixed_states())


def assert_cut_well_defined(results, cap, budget):
    """From the mirror alone: (smallest weight gap at a bond the cap cuts, smallest distance of a tail sum from the budget's
    threshold in units of the budget)."""
    gap, dist = np.inf, np.inf
    for out, _, sigmas in results:
        dims = out.bond_dims()
        for k, s in enumerate(sigmas):
            w, m = s * s, int(dims[k + 1])
            total = float(w.sum())
            assert np.all(s > 1e-12 * np.sqrt(total)), "no value near value_of_zero: the zero rule cuts nothing here"
            if m == len(s):
                continue
            if budget > 0.0:
                tail = float(w[m:][::-1].sum())
                dist = min(dist, (budget * total - tail) / (budget * total), (tail + float(w[m - 1]) - budget * total) / (budget * total))
            else:
                assert m == cap
                gap = min(gap, float(w[m - 1] - w[m]) / total)
    assert gap >= 1e-6 and dist >= 1e-9, (gap, dist)
    return gap, dist


def diag_overlaps(ctx, a, b):
    """(z_i = <a_i|b_i>, <a_i|a_i>, <b_i|b_i>) of two sets of equal length."""
    return np.diag(ctx.overlaps(a, b)).copy(), np.diag(ctx.overlaps(a, a)).real.copy(), np.diag(ctx.overlaps(b, b)).real.copy()


def infidelities(ctx, a, b):
    z, na, nb = diag_overlaps(ctx, a, b)
    return 1.0 - np.abs(z) ** 2 / (na * nb)


@pytest.fixture(scope="module")
def runs(gpu_ctx):
    """The mixed set on the device and every case compressed once: {"xs": set, case: (set, info)}."""
    out = {"xs": gpu_ctx.upload(list(mixed_states()))}
    for case, (cap, budget) in CASES.items():
        out[case] = gpu_ctx.compress(out["xs"], max_bond=cap, max_discard=budget, info=True)
    yield out
    for v in out.values():
        (v[0] if isinstance(v, tuple) else v).close()


# ---- 1. against the host mirror -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_agrees_with_the_host_mirror(gpu_ctx, runs, case):
    cap, budget = CASES[case]
    ref = mirror(case)
    gap, dist = assert_cut_well_defined(ref, cap, budget)
    cs, info = runs[case]
    ref_dims = np.stack([m.bond_dims() for m, _, _ in ref])
    assert info["bond_dims"].dtype == np.int32 and np.array_equal(info["bond_dims"], ref_dims) and np.array_equal(cs.dims, ref_dims)
    if case == "cap200":
        assert np.array_equal(ref_dims, np.stack([m.bond_dims() for m in mixed_states()]))
    else:
        assert ref_dims.max() < 128
    e_f = float(np.abs(info["fidelity"] - np.array([m.fidelity for m, _, _ in ref])).max())
    e_d = float(np.abs(info["discarded"] - np.stack([d for _, d, _ in ref])).max())
    with gpu_ctx.upload([m for m, _, _ in ref]) as ms:
        infid = float(np.abs(infidelities(gpu_ctx, ms, cs)).max())
    print(f"compress {case}: bonds up to {ref_dims.max()}, smallest gap {gap:.2e}, threshold distance {dist:.2e}; |d fidelity| = {e_f:.3e}, "
          f"|d discarded| = {e_d:.3e}, infidelity device vs mirror = {infid:.3e}")
    assert e_f <= 1e-12 and e_d <= 1e-12
    assert infid <= 1e-11


# ---- 2. identity, norm, Eckart-Young, spectra of the result -------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_identity_norm_and_bound(gpu_ctx, runs, case):
    xs = runs["xs"]
    cs, info = runs[case]
    z, nx, nc = diag_overlaps(gpu_ctx, xs, cs)
    e_id = float(np.abs((1.0 - np.abs(z) ** 2 / (nx * nc)) - (1.0 - info["fidelity"])).max())
    e_n = float(np.abs(nc / nx - 1.0).max())
    assert np.abs(info["fidelity"] - np.prod(1.0 - info["discarded"], axis=1)).max() < 1e-14
    assert np.all(info["discarded"] >= 0.0) and np.all(info["fidelity"] <= 1.0) and np.all(info["fidelity"] > 0.0)
    dims = info["bond_dims"]
    worst = np.inf
    for i, lam in enumerate(original_spectra()):  # Eckart-Young: no state of these bonds is closer
        bound = max(float(w[dims[i, k + 1]:][::-1].sum()) for k, w in enumerate(lam))
        worst = min(worst, (1.0 - info["fidelity"][i]) - bound)
        assert 1.0 - info["fidelity"][i] >= bound - 1e-13
    S = gpu_ctx.bond_spectra(cs)
    assert S.shape == (6, 19, dims[:, 1:-1].max())  # no weight beyond the new bonds
    assert np.abs(S.sum(-1) - 1.0).max() < 1e-12
    for i in range(6):
        for k in range(1, 20):
            assert np.all(S[i, k - 1, dims[i, k]:] == 0.0)
    print(f"compress {case}: identity holds to {e_id:.3e}, norm kept to {e_n:.3e}, smallest slack over the Eckart-Young bound {worst:.3e}")
    assert e_id <= 1e-12 and e_n <= 1e-12
    if CASES[case][1] > 0.0:
        assert np.all(info["discarded"] <= CASES[case][1])


def test_no_truncation_keeps_the_gram(gpu_ctx, runs):
    cs, info = runs["cap200"]
    assert np.all(info["discarded"] < 1e-30) and np.abs(info["fidelity"] - 1.0).max() < 1e-15
    K0, K1 = gpu_ctx.gram(runs["xs"]), gpu_ctx.gram(cs)
    scale = np.sqrt(np.outer(np.diag(K0), np.diag(K0)))
    err = float(np.abs((K1 - K0) / scale).max())
    print(f"gram of the set compressed without truncation: max |dK| / sqrt(K_ii K_jj) = {err:.3e}")
    assert err <= 1e-12


# ---- 3. short chains ----------------------------------------------------------------------------------------------------
def test_short_chains(gpu_ctx):
    rng = np.random.default_rng(8)
    for prof in ([1, 1], [1, 2, 1], [1, 1, 1], [1, 2, 2, 1], [1, 2, 1, 1], [1, 1, 2, 1]):
        n = len(prof) - 1
        states = [scrambled(Q.random_mps(n, prof, rng), rng, scale=1.0 + i) for i in range(3)]
        for cap in (None, 1):
            ref = [m.compress(max_bond=cap) for m in states]
            with gpu_ctx.upload(states) as xs:
                cs, info = gpu_ctx.compress(xs, max_bond=cap, info=True)
                with cs:
                    got = cs.download()
                    assert np.array_equal(cs.dims, np.stack([m.bond_dims() for m, _ in ref]))
                    assert info["discarded"].shape == (3, n - 1) and info["fidelity"].shape == (3,)
                    assert np.abs(info["fidelity"] - [m.fidelity for m, _ in ref]).max() <= 1e-12
                    if n > 1:
                        assert np.abs(info["discarded"] - np.stack([d for _, d in ref])).max() <= 1e-12
                    for g, (m, _), x in zip(got, ref, states):
                        a, b = dense_state(g.tensors), dense_state(m.tensors)
                        assert np.abs(a * np.vdot(a, b) / abs(np.vdot(a, b)) - b).max() < 1e-12 * np.linalg.norm(b)
                        if n == 1:  # a one-site chain is copied
                            assert np.array_equal(g.tensors[0], x.tensors[0]) and np.all(info["fidelity"] == 1.0)


# ---- 4. downloaded states -----------------------------------------------------------------------------------------------
def isometry_error(mps) -> float:
    worst = 0.0
    for t in mps.tensors[:-1]:
        mat = t.reshape(-1, t.shape[2])
        worst = max(worst, float(np.abs(mat.conj().T @ mat - np.eye(mat.shape[1])).max()))
    return worst


def test_downloaded_golden_states(gpu_ctx):
    """The 9-site golden states (bonds up to 16) cut at 3 and at 5: the tensors that come back are isometries and the same vectors
    as the mirror's up to a phase.  The amplitudes' tolerance: a subspace angle of at most 1e-15 / gap per bond, gap >= 1e-6
    asserted from the mirror, over 8 bonds -- 1e-8 of the norm."""
    xs_, ys_, _ = golden_mps_sets()
    states = [Q.MPS(t) for t in xs_ + ys_]
    for cap in (3, 5):
        ref = [m._compress(cap, 0.0, 1e-16) for m in states]
        gap, _ = assert_cut_well_defined(ref, cap, 0.0)
        with gpu_ctx.upload(states) as xs, gpu_ctx.compress(xs, max_bond=cap) as cs:
            got = cs.download()
            back = xs.download()
            assert np.array_equal(cs.dims, np.stack([m.bond_dims() for m, _, _ in ref])) and cs.dims.max() == cap
        assert all(np.array_equal(a, b) for x, m in zip(back, states) for a, b in zip(x.tensors, m.tensors))  # download of an upload
        worst_iso, worst_amp = 0.0, 0.0
        for g, (m, _, _) in zip(got, ref):
            assert [t.shape for t in g.tensors] == [t.shape for t in m.tensors]
            worst_iso = max(worst_iso, isometry_error(g))
            a, b = dense_state(g.tensors), dense_state(m.tensors)
            worst_amp = max(worst_amp, float(np.abs(a * np.vdot(a, b) / abs(np.vdot(a, b)) - b).max() / np.linalg.norm(b)))
        print(f"downloaded golden states cut at {cap} (gap {gap:.2e}): isometries to {worst_iso:.3e}, amplitudes vs mirror {worst_amp:.3e}")
        assert worst_iso <= 1e-12 and worst_amp <= 1e-8


def test_downloaded_ansatz_states(gpu_ctx):
    """Host-built 12-qubit ansatz states (bonds 40 to 58, Schmidt weights down to 1e-32 and nearly degenerate pairs of them, so
    the kept subspace of a cut is not unique and the vectors are not compared with the mirror's): the downloaded tensors are
    isometries, and the identity and the norm hold on the dense vectors."""
    ans = Q.KernelStateAnsatz(12, 3, 1.0, Q.entanglement_graph(12, 2))
    X = np.random.default_rng(5).uniform(0.0, 2.0, (3, 12))
    states = [Q.simulate(ans.circuit_for_data(x), 1.0) for x in X]
    assert min(m.max_bond() for m in states) >= 32
    with gpu_ctx.upload(states) as xs:
        cs, info = gpu_ctx.compress(xs, max_bond=4, info=True)
        with cs:
            got = cs.download()
    assert info["bond_dims"].max() == 4 and info["fidelity"].max() < 1.0 - 1e-6  # (the mirror: 1 - fidelity = 2.5e-4, 2.9e-4, 5.9e-5)
    for i, (g, m) in enumerate(zip(got, states)):
        a, b = dense_state(g.tensors), dense_state(m.tensors)
        na, nb = np.vdot(a, a).real, np.vdot(b, b).real
        e_id = abs((1.0 - abs(np.vdot(a, b)) ** 2 / (na * nb)) - (1.0 - info["fidelity"][i]))
        print(f"downloaded ansatz state {i} cut at 4: 1 - fidelity = {1.0 - info['fidelity'][i]:.3e}, identity to {e_id:.3e}, "
              f"norm to {abs(na / nb - 1.0):.3e}, isometries to {isometry_error(g):.3e}")
        assert e_id <= 1e-12 and abs(na / nb - 1.0) <= 1e-12 and isometry_error(g) <= 1e-12


# ---- 5. gauge invariance, rank-deficient sets ---------------------------------------------------------------------------
def test_gauge_invariance(gpu_ctx, runs):
    rng = np.random.default_rng(12)
    again = [scrambled(m, rng, scale=0.5) for m in mixed_states()]
    for case in ("cap16", "budget1e-3"):
        cap, budget = CASES[case]
        with gpu_ctx.upload(again) as ys, gpu_ctx.compress(ys, max_bond=cap, max_discard=budget) as cy:
            assert np.array_equal(cy.dims, runs[case][0].dims)
            infid = float(np.abs(infidelities(gpu_ctx, runs[case][0], cy)).max())
        print(f"compress {case} after another gauge change on every bond: infidelity = {infid:.3e}")
        assert infid <= 1e-10


def test_rank_deficient_set(gpu_ctx):
    """Bonds 1 and 3 wider than the Schmidt rank, by a gauge of cond <= 4: the set comes back at the ranks.  value_of_zero = 1e-12:
    the gauge leaves rounding of about 1e-15 of the norm in the directions a bond does not need."""
    rng = np.random.default_rng(13)
    prod = Q.simulate(Q.BoundCircuit.from_gates(5, [("Ry", [0], [0.3]), ("Rx", [1], [-0.7]), ("H", [2], []), ("Ry", [3], [1.2]), ("Rx", [4], [0.4])]), 1 - 1e-16)
    xx = Q.simulate(Q.BoundCircuit.from_gates(5, [("XXPhase", [0, 1], [0.3]), ("XXPhase", [2, 3], [0.6])]), 1 - 1e-16)
    full = Q.random_mps(5, [1, 2, 4, 4, 2, 1], rng)
    base = [prod, xx, full]
    assert [list(m.bond_dims()) for m in base[:2]] == [[1] * 6, [1, 2, 1, 2, 1, 1]]
    for grow, big_base in ((1, base), (3, base), (3, [Q.random_mps(20, PROFILES[k], rng) for k in range(3)])):
        states = [scrambled(m, rng, grow=grow) for m in big_base]
        with gpu_ctx.upload(big_base) as xs, gpu_ctx.upload(states) as ys:
            cs, info = gpu_ctx.compress(ys, value_of_zero=1e-12, info=True)
            with cs:
                assert np.array_equal(ys.dims[:, 1:-1], xs.dims[:, 1:-1] + grow)
                assert np.array_equal(cs.dims, xs.dims)
                assert info["discarded"].max() < 1e-24 and np.abs(info["fidelity"] - 1.0).max() < 1e-15
                infid = float(np.abs(infidelities(gpu_ctx, xs, cs)).max())
                ref_dims = np.stack([m.compress(value_of_zero=1e-12)[0].bond_dims() for m in states])
                assert np.array_equal(ref_dims, cs.dims)
        print(f"rank-deficient set, bonds {grow} wider than the rank (up to {int(ys.dims.max())}): infidelity to the original = {infid:.3e}")
        assert infid <= 1e-12


# ---- 6. bit guarantees --------------------------------------------------------------------------------------------------
def image_bytes(s):
    n, _, _, offs = s.image()
    planes = np.empty(n, dtype=np.float64)
    s.copy_image(planes.ctypes.data, n)
    bounds = list(offs[:, 0]) + [n]
    return [planes[bounds[i]:bounds[i + 1]].tobytes() for i in range(len(s))]


def test_bit_guarantees(gpu_ctx, runs):
    for case in ("cap17", "budget1e-3"):
        cap, budget = CASES[case]
        cs, info = runs[case]
        whole = image_bytes(cs)
        c2, info2 = gpu_ctx.compress(runs["xs"], max_bond=cap, max_discard=budget, info=True)  # twice in a row
        with c2:
            assert image_bytes(c2) == whole
            assert np.array_equal(info2["fidelity"], info["fidelity"]) and np.array_equal(info2["discarded"], info["discarded"])
        for i in (0, 1, 5):  # alone
            with gpu_ctx.upload([mixed_states()[i]]) as x1:
                c1, info1 = gpu_ctx.compress(x1, max_bond=cap, max_discard=budget, info=True)
                with c1:
                    assert image_bytes(c1)[0] == whole[i]
                    assert info1["fidelity"][0] == info["fidelity"][i] and np.array_equal(info1["discarded"][0], info["discarded"][i])


def test_more_states_than_workgroups(gpu_ctx):
    """600 six-site states: more than the two workgroups per compute unit, so a workgroup takes a second state after its first
    (its workspace and LDS words are reused).  States of the middle and the end are bit-equal to the same state alone and agree
    with the mirror."""
    rng = np.random.default_rng(21)
    profs = ([1, 2, 4, 8, 4, 2, 1], [1, 2, 3, 5, 4, 2, 1], [1, 2, 4, 5, 3, 2, 1])
    states = [scrambled(Q.random_mps(6, profs[i % 3], rng), rng) for i in range(600)]
    with gpu_ctx.upload(states) as xs:
        cs, info = gpu_ctx.compress(xs, max_bond=3, info=True)
        with cs:
            whole = image_bytes(cs)
            assert cs.dims.max() == 3
    for i in (0, 299, 511, 512, 599):
        m, d = states[i].compress(max_bond=3)
        assert np.array_equal(info["bond_dims"][i], m.bond_dims())
        assert abs(info["fidelity"][i] - m.fidelity) <= 1e-12 and np.abs(info["discarded"][i] - d).max() <= 1e-12
        with gpu_ctx.upload([states[i]]) as x1:
            c1, info1 = gpu_ctx.compress(x1, max_bond=3, info=True)
            with c1:
                assert image_bytes(c1)[0] == whole[i] and info1["fidelity"][0] == info["fidelity"][i]


# ---- 7. rejections ------------------------------------------------------------------------------------------------------
def test_rejections(gpu_ctx):
    rng = np.random.default_rng(0)
    L = engine.lib()
    C = engine.C
    QK_EINVAL = -1

    def call(ctx_h, set_h, cap, budget, zero, with_out=True):
        h = engine._P()
        rc = L.qk_mps_set_compress(ctx_h, set_h, cap, budget, zero, C.byref(h) if with_out else None, None, None)
        msg = (L.qk_last_error() or b"").decode()
        assert not h.value
        return rc, msg

    with gpu_ctx.upload([Q.random_mps(4, [1, 2, 4, 2, 1], rng)]) as s, s.to_f32() as s32:
        for args, text in (((None, s.handle, 0, 0.0, 0.0), "ctx is null"), ((gpu_ctx._h, None, 0, 0.0, 0.0), "src is null"),
                           ((gpu_ctx._h, s32.handle, 0, 0.0, 0.0), "complex64"), ((gpu_ctx._h, s.handle, -1, 0.0, 0.0), "max_bond"),
                           ((gpu_ctx._h, s.handle, 0, -1e-3, 0.0), "max_discard"), ((gpu_ctx._h, s.handle, 0, float("nan"), 0.0), "max_discard"),
                           ((gpu_ctx._h, s.handle, 0, float("inf"), 0.0), "max_discard"), ((gpu_ctx._h, s.handle, 0, 0.0, -1.0), "value_of_zero"),
                           ((gpu_ctx._h, s.handle, 0, 0.0, float("nan")), "value_of_zero")):
            rc, msg = call(*args)
            assert rc == QK_EINVAL and text in msg and "qk_mps_set_compress" in msg, (args, rc, msg)
        rc, msg = call(gpu_ctx._h, s.handle, 0, 0.0, 0.0, with_out=False)
        assert rc == QK_EINVAL and "out is null" in msg
        with engine.Context(0) as other:
            rc, msg = call(other._h, s.handle, 0, 0.0, 0.0)
            assert rc == QK_EINVAL and "another context" in msg
        with pytest.raises(engine.QkError, match="max_bond"):
            gpu_ctx.compress(s, max_bond=-2)
        with pytest.raises(ValueError, match="max_bond"):
            gpu_ctx.compress(s, max_bond=2.5)
        with gpu_ctx.compress(s) as ok:  # fidelity and discarded may be NULL; src is untouched
            assert np.array_equal(ok.dims, s.dims) and np.array_equal(gpu_ctx.gram(s), gpu_ctx.gram(s))
    wide = [1, 2, 4, 8, 16, 32, 64, 128, 256, 513, 256, 128, 64, 32, 16, 8, 4, 2, 1]
    big = Q.MPS([np.zeros((wide[k], 2, wide[k + 1]), dtype=np.complex128) for k in range(len(wide) - 1)])
    with gpu_ctx.upload([big]) as sb:  # rejected on the host, before anything runs on the device
        rc, msg = call(gpu_ctx._h, sb.handle, 0, 0.0, 0.0)
        assert rc == QK_EINVAL and "513" in msg and "512" in msg
    zero = Q.MPS([np.zeros((1, 2, 2), dtype=np.complex128), np.zeros((2, 2, 1), dtype=np.complex128)])
    one = Q.random_mps(2, [1, 2, 1], rng)
    with gpu_ctx.upload([one, zero]) as sz:  # a state of norm 0 is reported and named
        with pytest.raises(engine.QkError, match="state 1 has norm 0"):
            gpu_ctx.compress(sz)


# ---- 8. build_capped_kernel_matrices ------------------------------------------------------------------------------------
def _capped_case():
    n = 8
    return Q.KernelStateAnsatz(n, 3, 1.0, Q.entanglement_graph(n, 2)), R.synthetic_features(7, n, 31), R.synthetic_features(4, n, 32)


def dk_bound(fx, fy):
    """|dK[j, i]| <= d (2 + d), d = dx_i + dy_j + dx_i dy_j, delta = sqrt(2 - 2 sqrt(fidelity)), for normalised states."""
    dx, dy = np.sqrt(2.0 - 2.0 * np.sqrt(fx)), np.sqrt(2.0 - 2.0 * np.sqrt(fy))
    d = dx[None, :] + dy[:, None] + dx[None, :] * dy[:, None]
    return d * (2.0 + d)


def check_capped(out, nx, ny, caps):
    K = out["K"]
    assert K.shape == (ny or nx, nx) and set(out["K_capped"]) == set(caps) == set(out["fidelity"]) == set(out["bond_dims"])
    top = max(out["bond_dims"][c].max() for c in caps)
    assert top == out["bond_dims"][max(caps)].max() and max(caps) >= top > min(caps)
    assert np.abs(out["K_capped"][max(caps)] - K).max() <= 1e-12
    for c in caps:
        fid, dims = out["fidelity"][c], out["bond_dims"][c]
        assert fid.shape == (nx + ny,) and dims.shape == (nx + ny, 9) and dims.max() <= c and np.all(fid <= 1.0)
        fx, fy = fid[:nx], (fid[nx:] if ny else fid[:nx])
        excess = float((np.abs(out["K_capped"][c] - K) - dk_bound(fx, fy)).max())
        print(f"build_capped_kernel_matrices cap {c}: min fidelity {fid.min():.6f}, max |dK| {np.abs(out['K_capped'][c] - K).max():.3e}, "
              f"largest |dK| - bound {excess:.3e}")
        assert excess <= 1e-12
    assert out["fidelity"][min(caps)].min() < 1.0 - 1e-6


def test_build_capped_kernel_matrices(gpu_ctx, monkeypatch):
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_capped_kernel_matrices, build_kernel_matrix

    monkeypatch.setenv("QK_BUILDER", "host")
    ans, X, Y = _capped_case()
    caps = (2, 4, 64)
    sym = build_capped_kernel_matrices(SingleComm(), ans, X, caps=caps, truncation_error=1e-16)
    check_capped(sym, 7, 0, caps)
    assert np.abs(sym["K"] - build_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16)).max() <= 1e-12
    xy = build_capped_kernel_matrices(SingleComm(), ans, X, Y, caps=caps, truncation_error=1e-16)
    check_capped(xy, 7, 4, caps)
    assert np.array_equal(xy["fidelity"][2][:7], sym["fidelity"][2])


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["QK_BUILDER"] = "host"
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from qml_cutensornet_amd.dist import TorchComm
        from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_capped_kernel_matrices
        from test_gpu_compress import _capped_case as case_

        ans, X, Y = case_()
        q.put((rank, build_capped_kernel_matrices(TorchComm(), ans, X, Y, caps=(2, 4, 64), truncation_error=1e-16)))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_build_capped_kernel_matrices_two_ranks(built, monkeypatch):
    import torch.multiprocessing as mp

    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_capped_kernel_matrices

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + ((os.getpid() + 733) % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert res[1] is None
    check_capped(res[0], 7, 4, (2, 4, 64))
    monkeypatch.setenv("QK_BUILDER", "host")
    ans, X, Y = _capped_case()
    one = build_capped_kernel_matrices(SingleComm(), ans, X, Y, caps=(2, 4, 64), truncation_error=1e-16)
    for c in (2, 4, 64):  # a state's compression does not depend on the share it is in
        assert np.array_equal(res[0]["fidelity"][c], one["fidelity"][c]) and np.array_equal(res[0]["bond_dims"][c], one["bond_dims"][c])
        assert np.abs(res[0]["K_capped"][c] - one["K_capped"][c]).max() <= 1e-12
