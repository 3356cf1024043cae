"""``MPS.compress`` -- the host mirror of the device's canonical truncation sweep -- against the dense state, and the pure-numpy
``engine.unpack_state`` against ``engine.pack_state``.

The yardstick is the dense vector: SVD truncation of the contracted state bond by bond (``dense_truncation``: ``_kept`` plus the
cap on the Schmidt values of the progressively truncated vector, what is kept scaled back to the norm).  Tolerances: 1e-13 on norms
and on an unchanged vector, 1e-12 on the fidelity identity, on isometries and on discarded weights (all float64 routes of at most
2^12 amplitudes; the measured values sit at 1e-15).

The rank-deficient states take ``value_of_zero=1e-12``: the gauge of ``scrambled`` (cond <= 4) leaves rounding of about 1e-15 of
the norm in the directions a bond does not need, so "the Schmidt rank" is defined only for a zero above that noise."""
import numpy as np
import pytest

import qml_cutensornet_amd as Q
from qml_cutensornet_amd import engine
from qml_cutensornet_amd.mps import _kept

PROFILE_CASES = [  # (bond profile of 12 sites, max_bond, max_discard)
    ([1, 2, 4, 8, 16, 32, 64, 32, 16, 8, 4, 2, 1], 16, 0.0),
    ([1, 2, 4, 8, 15, 17, 33, 17, 16, 8, 4, 2, 1], 8, 0.0),
    ([1, 2, 4, 8, 16, 32, 48, 32, 16, 8, 4, 2, 1], None, 1e-3),
]


def dense_state(tensors) -> np.ndarray:
    psi = np.asarray(tensors[0])
    for t in tensors[1:]:
        psi = np.tensordot(psi, t, axes=(psi.ndim - 1, 0))
    return psi.reshape(-1)


def scrambled(mps, rng, grow=0, scale=3.7):
    """The bounded gauge of tests/test_entanglement_host.py (G = U diag(d) V, d in [0.5, 2]) on every bond, here with ``grow`` more
    columns than the bond has: G is chi x (chi + grow) with orthonormal rows of V, and its pseudo-inverse goes into the next
    site, so the state is the same (times ``scale``) and every bond is ``grow`` wider than its rank allows."""
    ts = [np.array(t, dtype=np.complex128) for t in mps.tensors]
    for k in range(1, len(ts)):
        chi = ts[k].shape[0]
        big = chi + grow
        u, _ = np.linalg.qr(rng.standard_normal((chi, chi)) + 1j * rng.standard_normal((chi, chi)))
        v, _ = np.linalg.qr(rng.standard_normal((big, big)) + 1j * rng.standard_normal((big, big)))
        d = rng.uniform(0.5, 2.0, chi)
        g = (u * d) @ v[:chi]  # chi x big
        gi = v[:chi].conj().T @ ((1.0 / d)[:, None] * u.conj().T)  # big x chi, g gi = 1
        ts[k - 1] = np.tensordot(ts[k - 1], g, axes=(2, 0))
        ts[k] = np.tensordot(gi, ts[k], axes=(1, 0))
    ts[0] = ts[0] * scale
    return Q.MPS(ts)


def dense_truncation(psi, n, max_bond, max_discard, value_of_zero):
    """(truncated dense vector, dims[0..n], discarded[n-1]) by one SVD of the dense vector per bond, left to right."""
    psi = np.array(psi, dtype=np.complex128)
    dims, disc = [1], []
    for k in range(1, n):
        u, s, vh = np.linalg.svd(psi.reshape(2 ** k, -1), full_matrices=False)
        w = s * s
        total = float(w.sum())
        m, _ = _kept(s, max_discard, value_of_zero * np.sqrt(total))
        if max_bond:
            m = min(m, int(max_bond))
        d = float(w[m:][::-1].sum()) / total
        psi = ((u[:, :m] * s[:m]) @ vh[:m]).reshape(-1) / np.sqrt(1.0 - d)
        dims.append(m)
        disc.append(d)
    return psi, dims + [1], np.array(disc)


def infidelity(a, b) -> float:
    return 1.0 - abs(np.vdot(a, b)) ** 2 / (np.vdot(a, a).real * np.vdot(b, b).real)


def check_isometries(mps, tol=1e-12):
    worst = 0.0
    for t in mps.tensors[:-1]:
        m = t.reshape(-1, t.shape[2])
        worst = max(worst, float(np.abs(m.conj().T @ m - np.eye(m.shape[1])).max()))
    assert worst < tol, worst
    return worst


@pytest.mark.parametrize("case", range(len(PROFILE_CASES)))
def test_compress_against_dense_svd_truncation(case):
    prof, cap, budget = PROFILE_CASES[case]
    n = len(prof) - 1
    rng = np.random.default_rng(40 + case)
    m = scrambled(Q.random_mps(n, prof, rng), rng) if case == 1 else Q.random_mps(n, prof, rng)
    psi = dense_state(m.tensors)
    out, disc = m.compress(max_bond=cap, max_discard=budget)
    got = dense_state(out.tensors)
    ref, dims, ref_disc = dense_truncation(psi, n, cap, budget, 1e-16)
    # rule parity: the cut of every bond is the one _kept and the cap make on the dense Schmidt values
    assert list(out.bond_dims()) == dims and max(dims) < max(prof)
    assert np.abs(disc - ref_disc).max() < 1e-12 and disc.max() > 1e-6
    if cap:
        assert max(dims) == cap
    else:
        assert np.all(disc <= budget) and disc.max() > 0.1 * budget
    assert infidelity(got, ref) < 1e-12
    # conventions
    norm0, norm1 = np.vdot(psi, psi).real, np.vdot(got, got).real
    assert abs(norm1 / norm0 - 1.0) < 1e-13
    check_isometries(out)
    assert abs(np.vdot(out.tensors[-1], out.tensors[-1]).real / norm0 - 1.0) < 1e-13  # the norm sits in the last site
    assert abs(out.fidelity - np.prod(1.0 - disc)) < 1e-15
    # the identity: nested projectors
    err = abs(infidelity(psi, got) - (1.0 - out.fidelity))
    print(f"profile {case}: new bonds {dims}, 1 - fidelity = {1.0 - out.fidelity:.6e}, identity holds to {err:.2e}")
    assert err < 1e-12
    # Eckart-Young against the spectra of the original
    lam = m.bond_spectra()
    bound = max(float(w[dims[k + 1]:].sum()) for k, w in enumerate(lam))
    assert bound > 1e-6 and 1.0 - out.fidelity >= bound - 1e-14


@pytest.mark.parametrize("case", range(len(PROFILE_CASES)))
def test_no_cap_no_budget_leaves_the_vector(case):
    prof, _, _ = PROFILE_CASES[case]
    n = len(prof) - 1
    rng = np.random.default_rng(50 + case)
    m = scrambled(Q.random_mps(n, prof, rng), rng)
    out, disc = m.compress()
    psi, got = dense_state(m.tensors), dense_state(out.tensors)
    assert list(out.bond_dims()) == prof and np.all(disc < 1e-30) and abs(out.fidelity - 1.0) < 1e-15
    assert np.abs(got * np.vdot(got, psi) / abs(np.vdot(got, psi)) - psi).max() < 1e-13 * np.linalg.norm(psi)
    check_isometries(out)
    again, _ = m.compress(max_bond=max(prof), max_discard=0.0)
    assert all(np.array_equal(a, b) for a, b in zip(again.tensors, out.tensors))


def test_rank_deficient_bonds_shrink_to_the_schmidt_rank():
    prod = Q.simulate(Q.BoundCircuit.from_gates(5, [("Ry", [0], [0.3]), ("Rx", [1], [-0.7]), ("H", [2], []), ("Ry", [3], [1.2]), ("Rx", [4], [0.4])]), 1 - 1e-16)
    xx = Q.simulate(Q.BoundCircuit.from_gates(4, [("XXPhase", [0, 1], [0.3]), ("XXPhase", [2, 3], [0.6])]), 1 - 1e-16)
    for m, ranks in ((prod, [1, 1, 1, 1, 1, 1]), (xx, [1, 2, 1, 2, 1])):
        assert list(m.bond_dims()) == ranks
        psi = dense_state(m.tensors)
        for grow in (1, 3):
            big = scrambled(m, np.random.default_rng(60 + grow), grow=grow)
            assert list(big.bond_dims()[1:-1]) == [r + grow for r in ranks[1:-1]]
            out, disc = big.compress(value_of_zero=1e-12)
            assert list(out.bond_dims()) == ranks
            got = dense_state(out.tensors) / 3.7
            assert np.abs(got * np.vdot(got, psi) / abs(np.vdot(got, psi)) - psi).max() < 1e-12
            assert disc.max() < 1e-24 and abs(out.fidelity - 1.0) < 1e-15
            check_isometries(out)


def test_compress_rejects_bad_arguments():
    m = Q.random_mps(4, [1, 2, 4, 2, 1], np.random.default_rng(0))
    for kw in ({"max_bond": -1}, {"max_bond": 2.5}, {"max_discard": -1e-3}, {"max_discard": np.nan}, {"value_of_zero": -1.0}, {"value_of_zero": np.inf}):
        with pytest.raises(ValueError):
            m.compress(**kw)
    zero = Q.MPS([np.zeros_like(t) for t in m.tensors])
    with pytest.raises(ValueError, match="norm 0"):
        zero.compress()
    one = Q.MPS([np.array([[[0.6], [0.8j]]])])
    out, disc = one.compress(max_bond=1)
    assert disc.shape == (0,) and out.fidelity == 1.0 and np.array_equal(out.tensors[0], one.tensors[0])


def test_unpack_state_inverts_pack_state(built):
    rng = np.random.default_rng(70)
    prof = [1, 2, 4, 8, 15, 16, 17, 33, 17, 16, 15, 8, 4, 2, 1]
    m = Q.random_mps(len(prof) - 1, prof, rng)
    assert {1, 2, 15, 16, 17, 33} <= set(prof)
    planes, offs = engine.pack_state(m)
    back = engine.unpack_state(planes, m.bond_dims(), offs)
    assert len(back) == len(m.tensors)
    for a, b in zip(back, m.tensors):
        assert a.dtype == np.complex128 and a.shape == b.shape and np.array_equal(a, b)
    with pytest.raises(ValueError, match="offsets"):
        engine.unpack_state(planes, m.bond_dims(), offs[:-1])
    with pytest.raises(ValueError, match="inside"):
        engine.unpack_state(planes[:-1], m.bond_dims(), offs)
