"""The general-gauge sets of tests/helpers.py (``gauge_sets``, ``gauge_set_300``) on the host (no GPU): the conditions on the inputs
and on the references that the GPU tests of the local sweeps and of the sampler rest on.

* The originals (``random_mps``: right-orthonormal) have R_k = 1 to 1e-13, which is why they do not test how a kernel reads R.
* The twins hold the same states with dense complex environments on both sides.  R_k of a twin is G^-1 G^-H and L_k is
  G^H L_k G of a normalised state (entries of order 1 / chi), times 3.7^2 for every second state, so the measure is relative: the
  largest off-diagonal entry, and the largest imaginary part, over the largest diagonal entry of the same matrix.  Both are >= 0.1
  for L_k and R_k at every bond of dimension >= 4 (measured minima: 0.1000086 for the 20-site twins, 0.129 for the 300-bond twins).
  A bond of dimension 2 or 3 is one draw of a 2 x 2 or 3 x 3 gauge and can come out nearly diagonal or nearly real (smallest here:
  0.0046 and 0.0011); such a bond fits any tile whichever way it is read, and the test only prints those figures.
* The references drift by at most 1e-13 between a twin and its original (measured: 2e-15 for the sweeps, 3e-14 for ``logp``).
* The sampler's cases: no draw of the mirror sits within 1e-9 of its threshold (a condition on seeds chosen here, not a
  tolerance; measured margins 5.6e-5 and 2.3e-4), and the twins draw the bits of their originals.
* The references are right on such states: one 18-qubit twin of ``gauge_set_300`` against its dense state vector.
* The references see the gauge: with R_{k+1} transposed, ``ref_local_paulis`` and the sampler's probabilities move by more than
  1e-3 on the twins and by less than 1e-13 on the originals."""
import functools

import numpy as np

from helpers import GAUGE_SAMPLE, SHOTS, environments, gauge_sample_case, gauge_set_300, gauge_sets
from qml_cutensornet_amd import engine
from test_gpu_pauli_strings import case_strings
from test_pauli_strings_host import pauli_strings_from_dense, ref_pauli_strings
from test_projected_dist_host import pair_dist_from_dense, ref_pair_paulis_dist
from test_projected_host import bloch_from_dense, dense, ref_local_paulis
from test_projected_pair_host import pair_from_dense, ref_pair_paulis
from test_sample_host import dense_of_mps, dense_probability

SETS = {"g20": gauge_sets, "g300": gauge_set_300}


def off_diagonal(M):
    return float(np.abs(M - np.diag(np.diag(M))).max())


@functools.lru_cache(maxsize=None)
def all_environments(name, which):
    return [environments(m.tensors) for m in SETS[name]()[which]]


def test_originals_have_a_trivial_right_environment():
    for name in SETS:
        worst = max(max(off_diagonal(r), float(np.abs(np.diag(r) - 1.0).max())) for _, R in all_environments(name, 0) for r in R[1:])
        print(f"{name} originals: max |R_k - 1| = {worst:.3e}")
        assert worst <= 1e-13


def test_twins_have_dense_complex_environments_on_both_sides():
    for name in SETS:
        wide, narrow = np.full(4, np.inf), np.full(4, np.inf)
        for L, R in all_environments(name, 1):
            for l, r in zip(L, R):
                if r.shape[0] < 2:
                    continue
                dl, dr = float(np.abs(np.diag(l)).max()), float(np.abs(np.diag(r)).max())
                fig = np.array([off_diagonal(r) / dr, np.abs(r.imag).max() / dr, off_diagonal(l) / dl, np.abs(l.imag).max() / dl])
                if r.shape[0] >= 4:
                    wide = np.minimum(wide, fig)
                else:
                    narrow = np.minimum(narrow, fig)
        print(f"{name} twins, smallest over the bonds of (off-diagonal R, |Im R|, off-diagonal L, |Im L|) / largest diagonal entry: "
              f"dimension >= 4: {wide}, dimension 2 and 3: {narrow}")
        assert np.all(wide >= 0.1), wide


def _drift(name, ref, indices=None):
    originals, twins = SETS[name]()
    worst = 0.0
    for i in range(len(twins)) if indices is None else indices:
        (vo, no), (vt, nt) = ref(originals[i].tensors), ref(twins[i].tensors)
        scale = 3.7**2 if i % 2 else 1.0
        worst = max(worst, float(np.abs(vt - vo).max()), abs(nt / scale - no) / no)
    return worst


@functools.lru_cache(maxsize=None)
def dist_reference(which, i):
    """``ref_pair_paulis_dist`` at max_dist = 3 (seconds per state: computed once)."""
    return ref_pair_paulis_dist(gauge_sets()[which][i].tensors, 3)


def test_references_do_not_drift_between_twin_and_original():
    S = case_strings(20, np.random.default_rng(135))
    dist = iter([dist_reference(w, i) for i in (0, 1) for w in (0, 1)])
    figures = {
        "ref_local_paulis": max(_drift("g20", ref_local_paulis), _drift("g300", ref_local_paulis)),
        "ref_pair_paulis": max(_drift("g20", ref_pair_paulis), _drift("g300", ref_pair_paulis)),
        "ref_pair_paulis_dist": _drift("g20", lambda t: next(dist), indices=(0, 1)),  # the states of the GPU test
        "ref_pauli_strings": _drift("g20", lambda t: ref_pauli_strings(t, S)),
    }
    print("reference drift, twin against original: " + ", ".join(f"{k}: {v:.3e}" for k, v in figures.items()))
    assert max(figures.values()) <= 1e-13


@functools.lru_cache(maxsize=None)
def mirror(name, which):
    """(bits, logp, margin) per state of a sampler case, or of the originals of its twins AT THE TWINS' global indices."""
    states, bases, seed, first = gauge_sample_case(name)
    if which == "originals":
        states = SETS[name]()[0]
    else:
        first = 0
    return [m.sample(SHOTS, bases=bases, seed=seed, state_index=first + i, logp=True, margin=True) for i, m in enumerate(states)]


def test_sampler_cases_are_well_conditioned_and_twins_draw_their_originals_bits():
    for name in GAUGE_SAMPLE:
        states, _, _, first = gauge_sample_case(name)
        case, orig = mirror(name, "case"), mirror(name, "originals")
        margin = min(o[2] for o in case + orig)
        twins = case[first:]
        dlp = max(float(np.abs(t[1] - o[1]).max()) for t, o in zip(twins, orig))
        print(f"{name}: smallest margin of the mirror = {margin:.3e} over {len(states)} states; logp drift twin vs original = {dlp:.3e}")
        assert margin >= 1e-9
        assert all(np.array_equal(t[0], o[0]) for t, o in zip(twins, orig))
        assert dlp <= 1e-13


def test_references_against_the_dense_vector_of_a_300_bond_twin():
    twin = gauge_set_300()[1][1]  # the scaled one
    n = len(twin)
    assert n == 18 and twin.max_bond() == 300
    psi = dense(twin)
    F, norm = ref_local_paulis(twin.tensors)
    Fd, nd = bloch_from_dense(psi, n)
    T, _ = ref_pair_paulis(twin.tensors)
    Td, _ = pair_from_dense(psi, n)
    # the distance reference takes minutes at bond 300: the 20-qubit twin the GPU test of the distance sweep uses, instead
    T3, _ = dist_reference(1, 1)
    T3d, _ = pair_dist_from_dense(dense(gauge_sets()[1][1]), 20, 3)
    S = case_strings(n, np.random.default_rng(300))
    V, _ = ref_pauli_strings(twin.tensors, S)
    Vd, _ = pauli_strings_from_dense(psi, n, S)
    errs = [float(np.abs(a - b).max()) for a, b in ((F, Fd), (T, Td), (T3, T3d), (V, Vd))]
    print(f"300-bond twin vs its dense vector: Bloch {errs[0]:.3e}, pairs {errs[1]:.3e}, pairs up to distance 3 (20-site twin) {errs[2]:.3e}, "
          f"strings {errs[3]:.3e}, norm {abs(norm - nd) / nd:.3e}")
    assert max(errs) < 1e-13 and abs(norm - nd) < 1e-13 * nd and abs(norm - 3.7**2) < 1e-12 * norm
    _, bases, seed, first = gauge_sample_case("g300")
    bits, lp, _ = mirror("g300", "case")[first + 1]
    exact = dense_probability(dense_of_mps(twin), bits[:16], bases[:16])
    assert np.all(np.abs(np.exp(lp[:16]) - exact) <= 1e-8 * exact)


# ---- the references see the gauge: R_{k+1} transposed ----------------------------------------------------------------------
def _bloch_with_r_transposed(tensors):
    """``ref_local_paulis`` with the right environment read transposed."""
    _, R = environments(tensors)
    norm = R[0][0, 0].real
    L = np.ones((1, 1), dtype=complex)
    F = np.zeros((len(tensors), 3))
    for k, A in enumerate(tensors):
        rho = np.einsum("lm,lsr,rq,mtq->st", L, A, R[k + 1].T, A.conj(), optimize=True) / norm
        F[k] = (2 * rho[0, 1].real, -2 * rho[0, 1].imag, (rho[0, 0] - rho[1, 1]).real)
        L = np.einsum("lm,lsr,msq->rq", L, A, A.conj(), optimize=True)
    return F


def _outcome_probabilities(m, transpose):
    """p(outcome 0) in X, Y and Z at every site, as ``MPS.sample`` forms it after a run of zeros in Z, with R_{k+1} as it is or
    transposed: (n, 3)."""
    _, R = environments(m.tensors)
    h = np.sqrt(0.5)
    v = np.ones(1, dtype=complex)
    out = []
    for k, A in enumerate(m.tensors):
        Rk = R[k + 1].T if transpose else R[k + 1]
        W0, W1 = v @ np.asarray(A)[:, 0], v @ np.asarray(A)[:, 1]
        row = []
        for a0, a1 in (((W0 + W1) * h, (W0 - W1) * h), ((W0 - 1j * W1) * h, (W0 + 1j * W1) * h), (W0, W1)):
            p0, p1 = (a0 @ Rk @ a0.conj()).real, (a1 @ Rk @ a1.conj()).real
            row.append(p0 / (p0 + p1))
        out.append(row)
        v = W0 / np.linalg.norm(W0)
    return np.array(out)


def test_a_transposed_right_environment_shows_on_the_twins_only():
    fig = {}
    for which, label in ((0, "originals"), (1, "twins")):
        states = [m for name in SETS for m in SETS[name]()[which]]
        fig[label] = (max(float(np.abs(_bloch_with_r_transposed(m.tensors) - ref_local_paulis(m.tensors)[0]).max()) for m in states),
                      max(float(np.abs(_outcome_probabilities(m, True) - _outcome_probabilities(m, False)).max()) for m in states))
    print(f"R transposed against R, Bloch vectors / outcome probabilities: originals {fig['originals'][0]:.3e} / {fig['originals'][1]:.3e}, "
          f"twins {fig['twins'][0]:.3e} / {fig['twins'][1]:.3e}")
    assert max(fig["originals"]) <= 1e-13
    assert min(fig["twins"]) >= 1e-3
