"""Per-bond entanglement spectra on the host: ``MPS.bond_spectra()`` against the dense SVD of the contracted state, analytic
states, and the numpy helpers ``bond_entropies``, ``cap_cost`` and ``schmidt_rank`` of the engine module.

Tolerances: 1e-12 on weights against the same tensors or the dense state (the float64 routes sit at 1e-15), 1e-10 for entropies.

The gauge matrices of ``scrambled`` are G = U diag(d) V with Haar-random unitaries U, V and d uniform in [0.5, 2], so
cond(G) <= 4.  The weights do not depend on the gauge, but a route through the environments (the device's) sees them through
Gram matrices of the gauge and loses eps cond(G)^2 -- measured in numpy on the 64-bond profile below: 1.4e-15 with this gauge,
2e-11 to 4e-8 with complex Gaussian matrices (cond 150 to 5500), where the QR/SVD route of ``MPS.bond_spectra`` still holds
2e-13.  The bounded gauge keeps the comparison at 1e-12 a statement about the code and not about the conditioning of the input."""
import numpy as np
import pytest

import qml_cutensornet_amd as Q
from qml_cutensornet_amd.engine import bond_entropies, cap_cost, schmidt_rank

RAGGED64 = [1, 2, 4, 8, 16, 32, 64, 32, 16, 8, 4, 2, 1]  # 12 sites


def dense_state(tensors) -> np.ndarray:
    psi = np.asarray(tensors[0])
    for t in tensors[1:]:
        psi = np.tensordot(psi, t, axes=(psi.ndim - 1, 0))
    return psi.reshape(-1)


def dense_spectra(psi, n) -> list:
    """Descending squared singular values (normalised) of the dense state across every interior cut."""
    out = []
    for k in range(1, n):
        s = np.linalg.svd(np.asarray(psi).reshape(2 ** k, -1), compute_uv=False)
        out.append(s * s / float((s * s).sum()))
    return out


def spectra_error(got, ref) -> float:
    """max |got - ref| over all bonds; the shorter of the two lists of a bond is zero-filled."""
    worst = 0.0
    for a, b in zip(got, ref):
        m = max(len(a), len(b))
        pa, pb = np.zeros(m), np.zeros(m)
        pa[: len(a)], pb[: len(b)] = a, b
        worst = max(worst, float(np.abs(pa - pb).max()))
    return worst


def scrambled(mps, rng, scale=3.7):
    """The same state times ``scale`` with G_k G_k^-1 inserted on every bond (G_k = U diag(d) V, cond <= 4): no site is
    orthonormal any more, on either side."""
    ts = [np.array(t) for t in mps.tensors]
    for k in range(1, len(ts)):
        chi = ts[k].shape[0]
        u, _ = np.linalg.qr(rng.standard_normal((chi, chi)) + 1j * rng.standard_normal((chi, chi)))
        v, _ = np.linalg.qr(rng.standard_normal((chi, chi)) + 1j * rng.standard_normal((chi, chi)))
        g = (u * rng.uniform(0.5, 2.0, chi)) @ v
        ts[k - 1] = np.tensordot(ts[k - 1], g, axes=(2, 0))
        ts[k] = np.tensordot(np.linalg.inv(g), ts[k], axes=(1, 0))
    ts[0] = ts[0] * scale
    return Q.MPS(ts)


def duplicated_column(rng, n=8, prof=(1, 2, 4, 8, 9, 8, 4, 2, 1), bond=4):
    """A state whose bond ``bond`` has one more column than its Schmidt rank: column 0 of the bond is split into two halves."""
    base = list(prof)
    base[bond] -= 1
    m = Q.random_mps(n, base, rng)
    ts = [np.array(t) for t in m.tensors]
    left, right = ts[bond - 1], ts[bond]
    ts[bond - 1] = np.concatenate([left, left[:, :, :1]], axis=2)
    half = right.copy()
    half[0] *= 0.5
    ts[bond] = np.concatenate([half, half[:1]], axis=0)
    return Q.MPS(ts), base[bond]


def ansatz_states(n, reps, count, seed, fidelity=1.0):
    """Host-built states of the ansatz at ``count`` points x ~ U(0, 2).  ``fidelity=1``: only singular values <= 1e-16 are dropped,
    so the bonds carry Schmidt weights down to 1e-32 (12 qubits x 3 layers: bonds 40 to 58)."""
    ans = Q.KernelStateAnsatz(n, reps, 1.0, Q.entanglement_graph(n, 2))
    X = np.random.default_rng(seed).uniform(0.0, 2.0, (count, n))
    return [Q.simulate(ans.circuit_for_data(x), fidelity) for x in X]


@pytest.fixture(scope="module")
def ragged():
    rng = np.random.default_rng(3)
    states = [Q.random_mps(12, RAGGED64, rng) for _ in range(2)]
    return states, [dense_spectra(dense_state(m.tensors), 12) for m in states], rng


# ---- MPS.bond_spectra against the dense SVD ------------------------------------------------------------------------------
def test_ragged_random_against_dense(ragged):
    states, refs, _ = ragged
    for m, ref in zip(states, refs):
        got = m.bond_spectra()
        assert [len(w) for w in got] == RAGGED64[1:-1]
        assert max(int((w >= 1e-3).sum()) for w in ref) >= 8
        err = spectra_error(got, ref)
        print(f"bond_spectra vs dense SVD (ragged, bond 64): max |d lambda| = {err:.3e}")
        assert err < 1e-12
        for w in got:
            assert abs(w.sum() - 1.0) < 1e-12 and np.all(np.diff(w) <= 0) and np.all(w >= 0)


def test_gauge_and_scale_do_not_change_the_weights(ragged):
    states, refs, rng = ragged
    for m, ref in zip(states, refs):
        sc = scrambled(m, np.random.default_rng(11))
        assert abs(np.vdot(dense_state(sc.tensors), dense_state(sc.tensors)).real - 3.7 ** 2) < 1e-9
        err = spectra_error(sc.bond_spectra(), ref)
        print(f"bond_spectra after a gauge change on every bond and a factor 3.7: max |d lambda| = {err:.3e}")
        assert max(int((w >= 1e-3).sum()) for w in ref) >= 8
        assert err < 1e-12


def test_rank_deficient_bond():
    m, rank = duplicated_column(np.random.default_rng(5))
    got = m.bond_spectra()
    ref = dense_spectra(dense_state(m.tensors), len(m))
    assert len(got[3]) == rank + 1
    assert got[3][rank:].max() < 1e-14
    assert spectra_error(got, ref) < 1e-12
    S = np.zeros((1, len(got), max(len(w) for w in got)))
    for k, w in enumerate(got):
        S[0, k, : len(w)] = w
    assert schmidt_rank(S, 1e-12)[0, 3] == rank
    assert np.array_equal(schmidt_rank(S, 1e-12)[0], [2, 4, 8, rank, 8, 4, 2])


def test_host_built_ansatz_states():
    for m in ansatz_states(12, 3, 3, 5):
        assert m.max_bond() >= 32
        ref = dense_spectra(dense_state(m.tensors), 12)
        assert int((ref[5] >= 1e-3).sum()) >= 2
        err = spectra_error(m.bond_spectra(), ref)
        print(f"bond_spectra vs dense SVD (12 qubits x 3 layers, bond {m.max_bond()}): max |d lambda| = {err:.3e}, "
              f"{int((ref[5] >= 1e-3).sum())} weights >= 1e-3 at the middle bond")
        assert err < 1e-12


# ---- analytic states -----------------------------------------------------------------------------------------------------
def product_state():
    gates = [("Ry", [0], [0.3]), ("Rx", [1], [-0.7]), ("H", [2], []), ("Ry", [3], [1.2]), ("Rx", [4], [0.4])]
    return Q.simulate(Q.BoundCircuit.from_gates(5, gates), 1 - 1e-16)


def xxphase_state(alpha, n=2, qubits=(0, 1)):
    return Q.simulate(Q.BoundCircuit.from_gates(n, [("XXPhase", list(qubits), [alpha])]), 1 - 1e-16)


def xx_weights(alpha):
    return np.array(sorted([np.cos(0.5 * np.pi * alpha) ** 2, np.sin(0.5 * np.pi * alpha) ** 2], reverse=True))


def test_product_state():
    for w in product_state().bond_spectra():
        assert len(w) == 1 and w[0] == 1.0


def test_xxphase():
    for alpha in (0.5, 0.3, 1.7):
        (w,) = xxphase_state(alpha).bond_spectra()
        assert np.abs(w - xx_weights(alpha)).max() < 1e-12
    (w,) = xxphase_state(0.5).bond_spectra()
    assert abs(bond_entropies(w) - np.log(2.0)) < 1e-10 and abs((w * w).sum() - 0.5) < 1e-12
    got = xxphase_state(0.3, 3, (0, 2)).bond_spectra()
    assert len(got) == 2
    for w in got:
        assert np.abs(w[:2] - xx_weights(0.3)).max() < 1e-12 and np.all(w[2:] < 1e-14)


# ---- helpers -------------------------------------------------------------------------------------------------------------
def test_bond_entropies():
    rng = np.random.default_rng(2)
    w = rng.uniform(0.0, 1.0, (3, 4, 9))
    w[..., 6:] = 0.0  # the zero fill
    w /= w.sum(axis=-1, keepdims=True)
    nz = w[..., :6]
    assert np.abs(bond_entropies(w) - (-(nz * np.log(nz)).sum(-1))).max() < 1e-10
    assert np.abs(bond_entropies(w, 2.0) - (-np.log((nz ** 2).sum(-1)))).max() < 1e-10
    assert np.abs(bond_entropies(w, 0.5) - 2.0 * np.log(np.sqrt(nz).sum(-1))).max() < 1e-10
    assert bond_entropies(w).shape == (3, 4)
    assert bond_entropies(np.array([1.0, 0.0, 0.0])) == 0.0 and bond_entropies(np.array([1.0, 0.0]), 2.0) == 0.0
    for bad in (0.0, -1.0, np.inf):
        with pytest.raises(ValueError, match="alpha"):
            bond_entropies(w, bad)


def test_cap_cost():
    rng = np.random.default_rng(4)
    w = np.sort(rng.uniform(0.0, 1.0, (2, 5, 8)), axis=-1)[..., ::-1]
    w /= w.sum(axis=-1, keepdims=True)
    for chi in (1, 3, 7):
        assert np.abs(cap_cost(w, chi) - w[..., chi:].sum(-1)).max() < 1e-15
        assert cap_cost(w, chi).shape == (2, 5)
    assert np.all(cap_cost(w, 8) == 0.0) and np.all(cap_cost(w, 50) == 0.0)
    assert np.abs(cap_cost(w, 1) - (1.0 - w[..., 0])).max() < 1e-15
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError, match="chi"):
            cap_cost(w, bad)
