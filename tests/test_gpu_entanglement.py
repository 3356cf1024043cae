"""Per-bond entanglement spectra and purities on the MI355X: qk_bond_spectra_host and qk_bond_purities_host against
``MPS.bond_spectra()`` on the same tensors (1e-12) and against exact state vectors (1e-10), their internal identities, analytic
states, the bit guarantees, the rejections, and ``build_entanglement_profile`` with one and two ranks.

Shapes: chains of 1, 2 and 3 sites; bonds of 1, 2, 15, 16, 17 (row padding), 47 and 48 (the switch of the Jacobi path), 63, 64, 65
and 128 (one, two and more 64-blocks of the GEMM), from ragged ``random_mps`` profiles; one set mixes three profiles, so tasks of
different sizes share every launch.  Measured on the MI355X: max |d lambda| 7.1e-15 and max |d purity| 2.3e-15 against the host
mirror (the gauge-scrambled set, bonds up to 128), 8.5e-16 against the dense SVD of the 14-qubit state (bond 126), 5.4e-12 against
exact state vectors for the built 8-qubit states (their truncation budget of 1e-16).  The gauge of the scrambled sets is the bounded one of tests/test_entanglement_host.py (its
docstring says why).  A comparison asserts that its states carry entanglement: a bond with at least 8 weights >= 1e-3 for the
random sets, at least 2 at the middle bond for the ansatz states."""
import os
import sys

import numpy as np
import pytest

import qml_cutensornet_amd as Q
from helpers import golden_mps_sets
from oracle import restatement as R
from qml_cutensornet_amd import engine
from test_entanglement_host import ansatz_states, dense_spectra, dense_state, product_state, scrambled, xx_weights, xxphase_state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 20 sites each; between them the bonds 1, 2, 15, 16, 17, 47, 48, 63, 64, 65, 128
PROFILES = [
    [1, 2, 4, 8, 15, 16, 17, 32, 47, 48, 63, 64, 65, 128, 64, 32, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 16, 31, 48, 64, 65, 33, 17, 9, 5, 3, 2, 1, 1, 1, 1, 1, 1],
    [1, 2, 4, 8, 15, 8, 4, 2, 1, 1, 2, 3, 5, 9, 17, 16, 8, 4, 2, 2, 1],
]


def host_reference(states):
    """(spectra (ns, n - 1, widest bond) zero-filled, purities, norms) from ``MPS.bond_spectra`` and the dense-free norm."""
    n = len(states[0])
    m = max(max(s.max_bond() for s in states), 1)
    S = np.zeros((len(states), n - 1, m))
    for i, s in enumerate(states):
        for k, w in enumerate(s.bond_spectra()):
            S[i, k, : len(w)] = w
    norms = []
    for s in states:
        L = np.ones((1, 1), dtype=complex)
        for t in s.tensors:
            L = np.einsum("ba,bsc,asd->cd", L, t, t.conj(), optimize=True)
        norms.append(L[0, 0].real)
    return S, (S * S).sum(-1), np.array(norms)


def device_values(ctx, states, max_values=None):
    with ctx.upload(states) as s:
        S, nrm = ctx.bond_spectra(s, max_values=max_values, norms=True)
        P, nrm_p = ctx.bond_purities(s, norms=True)
        F, nrm_f = ctx.local_paulis(s, norms=True)
    assert np.array_equal(nrm, nrm_f) and np.array_equal(nrm_p, nrm_f)  # the bits of local_paulis
    return S, P, nrm


def check_identities(states, S, P):
    ns, n = len(states), len(states[0])
    assert S.shape[:2] == (ns, n - 1) and P.shape == (ns, n - 1) and S.dtype == np.float64
    assert np.abs(S.sum(-1) - 1.0).max() < 1e-12
    assert np.abs(P - (S * S).sum(-1)).max() < 1e-12
    assert np.all(S >= 0.0) and np.all(np.diff(S, axis=-1) <= 0.0)
    for i, s in enumerate(states):
        chi = s.bond_dims()
        for k in range(1, n):
            assert np.all(S[i, k - 1, chi[k]:] == 0.0)
            if chi[k] == 1:
                assert S[i, k - 1, 0] == 1.0


def check_against_host(ctx, states, label, min_weights=8, middle=False, tol=1e-12):
    S, P, nrm = device_values(ctx, states)
    ref, ref_p, ref_n = host_reference(states)
    assert S.shape == ref.shape
    for r in ref:
        counts = (r >= 1e-3).sum(-1)
        assert (counts[len(counts) // 2] if middle else counts.max()) >= min_weights
    e_s, e_p = float(np.abs(S - ref).max()), float(np.abs(P - ref_p).max())
    print(f"bond spectra vs MPS.bond_spectra {label}: {len(states)} states, bonds up to {ref.shape[2]}, max |d lambda| = {e_s:.3e}, max |d purity| = {e_p:.3e}")
    assert e_s < tol and e_p < tol
    assert np.abs(nrm / ref_n - 1.0).max() < 1e-12
    check_identities(states, S, P)
    return S, P


@pytest.fixture(scope="module")
def mixed_states():
    rng = np.random.default_rng(7)
    return [scrambled(Q.random_mps(20, PROFILES[k % 3], rng), rng) for k in range(6)]


# ---- 1. against the host mirror on the same tensors ---------------------------------------------------------------------
def test_golden_sets(gpu_ctx):
    xs, ys, _ = golden_mps_sets()
    check_against_host(gpu_ctx, [Q.MPS(t) for t in xs + ys], "(golden sets)", min_weights=3)


def test_ragged_random_mixed_profiles(gpu_ctx, mixed_states):
    check_against_host(gpu_ctx, mixed_states, "(three ragged profiles, gauge-scrambled, scaled by 3.7)")


def test_ragged_random_right_orthonormal(gpu_ctx):
    rng = np.random.default_rng(9)
    check_against_host(gpu_ctx, [Q.random_mps(20, PROFILES[0], rng)], "(bond 128, right-orthonormal: R_k = 1)")


def test_host_built_12_qubits(gpu_ctx):
    check_against_host(gpu_ctx, ansatz_states(12, 3, 3, 5), "(host-built, 12 qubits x 3 layers)", min_weights=2, middle=True)


def test_device_built_states(gpu_ctx):
    """States of the device builder, downloaded and uploaded again: its sites are isometries to about 1e-11 only, so an environment
    is 1 + 1e-11 of noise -- nearly degenerate columns, which the factorisation must still diagonalise (a Jacobi sweep that stops
    early there cost 2e-11 of a weight on the 60-qubit benchmark set).  Measured on the MI355X: bonds up to 79, max |d lambda|
    2.4e-14, max |d purity| 2.2e-15."""
    ans = Q.KernelStateAnsatz(16, 4, 1.0, Q.entanglement_graph(16, 2))
    X = R.synthetic_features(6, 16, 5)
    states, info = gpu_ctx.build_mps([ans.circuit_for_data(x) for x in X], 1 - 1e-16, max_bond=320)
    gpu_ctx.trim()
    assert not info["dropped"] and max(m.max_bond() for m in states) >= 32
    check_against_host(gpu_ctx, states, "(device-built, 16 qubits x 4 layers)", min_weights=2)


def test_host_built_14_qubits_against_dense_svd(gpu_ctx):
    m = ansatz_states(14, 4, 5, 5)[4]  # built without a truncation budget: bond 126, Schmidt weights down to 1e-32
    assert m.max_bond() >= 120
    ref = dense_spectra(dense_state(m.tensors), 14)
    assert int((ref[6] >= 1e-3).sum()) >= 2
    S, P, _ = device_values(gpu_ctx, [m])
    err = max(float(np.abs(S[0, k, : len(w)] - w[: S.shape[2]]).max()) for k, w in enumerate(ref))
    err_p = max(abs(P[0, k] - float((w * w).sum())) for k, w in enumerate(ref))
    print(f"bond spectra vs dense SVD (14 qubits x 4 layers, bond {m.max_bond()}): max |d lambda| = {err:.3e}, max |d purity| = {err_p:.3e}")
    assert err < 1e-10 and err_p < 1e-10
    check_identities([m], S, P)
    s1 = engine.bond_entropies(S)[0]
    want = np.array([-(w[w > 0] * np.log(w[w > 0])).sum() for w in ref])
    assert np.abs(s1 - want).max() < 1e-10


# ---- 2. short chains, max_values ----------------------------------------------------------------------------------------
def test_short_chains(gpu_ctx):
    rng = np.random.default_rng(8)
    one = [Q.random_mps(1, [1, 1], rng) for _ in range(2)]
    with gpu_ctx.upload(one) as s:
        S, nrm = gpu_ctx.bond_spectra(s, norms=True)
        P = gpu_ctx.bond_purities(s)
        assert S.shape == (2, 0, 1) and P.shape == (2, 0)
        assert np.array_equal(nrm, gpu_ctx.local_paulis(s, norms=True)[1])
    for prof in ([1, 2, 1], [1, 1, 1], [1, 2, 2, 1], [1, 2, 1, 1], [1, 1, 2, 1]):
        states = [Q.random_mps(len(prof) - 1, prof, rng) for _ in range(3)]
        S, P, _ = device_values(gpu_ctx, states)
        ref, ref_p, _ = host_reference(states)
        assert np.abs(S - ref).max() < 1e-12 and np.abs(P - ref_p).max() < 1e-12
        check_identities(states, S, P)


def test_max_values_returns_the_leading_columns(gpu_ctx, mixed_states):
    with gpu_ctx.upload(mixed_states) as s:
        full = gpu_ctx.bond_spectra(s)
        assert full.shape == (6, 19, 128)
        for m in (1, 16, 47, 200):
            part = gpu_ctx.bond_spectra(s, max_values=m)
            assert part.shape == (6, 19, m)
            assert np.array_equal(part[..., : min(m, 128)], full[..., :m])
            assert np.all(part[..., 128:] == 0.0)


# ---- 3. analytic states -------------------------------------------------------------------------------------------------
def test_analytic_states(gpu_ctx):
    S, P, _ = device_values(gpu_ctx, [product_state()])
    assert S.shape == (1, 4, 1) and np.all(S == 1.0) and np.abs(P - 1.0).max() < 1e-12
    for alpha in (0.5, 0.3):
        S, P, _ = device_values(gpu_ctx, [xxphase_state(alpha)])
        assert np.abs(S[0, 0] - xx_weights(alpha)).max() < 1e-12
        assert abs(P[0, 0] - (xx_weights(alpha) ** 2).sum()) < 1e-12
    S, P, _ = device_values(gpu_ctx, [xxphase_state(0.5)])
    assert abs(engine.bond_entropies(S)[0, 0] - np.log(2.0)) < 1e-10 and abs(P[0, 0] - 0.5) < 1e-12
    S, _, _ = device_values(gpu_ctx, [xxphase_state(0.3, 3, (0, 2))])
    assert S.shape[:2] == (1, 2)
    for k in range(2):
        assert np.abs(S[0, k, :2] - xx_weights(0.3)).max() < 1e-12 and np.all(S[0, k, 2:] < 1e-14)


# ---- 4. bit guarantees --------------------------------------------------------------------------------------------------
def test_bit_guarantees(gpu_ctx, mixed_states):
    def both(states, m=128):
        with gpu_ctx.upload(states) as s:
            return gpu_ctx.bond_spectra(s, max_values=m), gpu_ctx.bond_purities(s), gpu_ctx.bond_spectra(s, max_values=m), gpu_ctx.bond_purities(s)

    S, P, S2, P2 = both(mixed_states)
    assert np.array_equal(S, S2) and np.array_equal(P, P2)  # repeated
    for i in (0, 4):
        Sa, Pa, _, _ = both([mixed_states[i]])
        assert np.array_equal(Sa[0], S[i]) and np.array_equal(Pa[0], P[i])  # alone
    order = [3, 0, 5, 1, 4, 2]
    Sr, Pr, _, _ = both([mixed_states[i] for i in order])
    assert np.array_equal(Sr, S[order]) and np.array_equal(Pr, P[order])  # reordered


def test_more_tasks_than_workgroups(gpu_ctx):
    """48 ragged 20-site states, 800 (state, bond) tasks: more than the two workgroups per compute unit that take them in
    turn, so a workgroup factorises several bonds one after the other -- 2, 17, 47, 48, 65 and 128 follow each other in its
    workspace, its LDS words and its table of clean block pairs.  Every state against the host mirror, and states from the
    middle and the end of the set bit-equal to the same state alone.  Measured on the MI355X: max |d lambda| 1.1e-14, max
    |d purity| 2.4e-15."""
    rng = np.random.default_rng(21)
    states = [scrambled(Q.random_mps(20, PROFILES[k % 3], rng), rng) for k in range(48)]
    n_tasks = sum(int((s.bond_dims()[1:-1] >= 2).sum()) for s in states)
    with gpu_ctx.upload(states) as s:
        assert n_tasks == 800  # the MI355X has 256 compute units: at most 512 workgroups
        S = gpu_ctx.bond_spectra(s)
        P = gpu_ctx.bond_purities(s)
    ref, ref_p, _ = host_reference(states)
    e_s, e_p = float(np.abs(S - ref).max()), float(np.abs(P - ref_p).max())
    print(f"bond spectra, {n_tasks} tasks in one launch: max |d lambda| = {e_s:.3e}, max |d purity| = {e_p:.3e}")
    assert e_s < 1e-12 and e_p < 1e-12
    check_identities(states, S, P)
    for i in (23, 24, 25, 47):  # one of each profile from the middle, and the last
        with gpu_ctx.upload([states[i]]) as s1:
            assert np.array_equal(gpu_ctx.bond_spectra(s1, max_values=128)[0], S[i])
            assert np.array_equal(gpu_ctx.bond_purities(s1)[0], P[i])


# ---- 5. rejections ------------------------------------------------------------------------------------------------------
def test_rejections(gpu_ctx):
    rng = np.random.default_rng(0)
    L = engine.lib()
    out = np.zeros((1, 3, 4))
    with gpu_ctx.upload([Q.random_mps(4, [1, 2, 4, 2, 1], rng)]) as s, s.to_f32() as s32:
        with pytest.raises(engine.QkError, match="complex64"):
            gpu_ctx.bond_spectra(s32)
        with pytest.raises(engine.QkError, match="complex64"):
            gpu_ctx.bond_purities(s32)
        for bad in (0, -3):
            with pytest.raises(engine.QkError, match="max_values"):
                gpu_ctx.bond_spectra(s, max_values=bad)
        with pytest.raises(ValueError, match="max_values"):
            gpu_ctx.bond_spectra(s, max_values=2.5)
        for args, name in (((None, s.handle, 4, out.ctypes.data, None), "ctx"), ((gpu_ctx._h, None, 4, out.ctypes.data, None), "set"),
                           ((gpu_ctx._h, s.handle, 4, None, None), "out")):
            with pytest.raises(engine.QkError, match=f"{name} is null"):
                engine._check(L.qk_bond_spectra_host(*args), "spectra")
            with pytest.raises(engine.QkError, match=f"{name} is null"):
                engine._check(L.qk_bond_purities_host(*(args[:2] + args[3:])), "purities")
        with engine.Context(0) as other:
            with pytest.raises(engine.QkError, match="set belongs to another context"):
                engine._check(L.qk_bond_spectra_host(other._h, s.handle, 4, out.ctypes.data, None), "spectra")
            with pytest.raises(engine.QkError, match="set belongs to another context"):
                engine._check(L.qk_bond_purities_host(other._h, s.handle, out.ctypes.data, None), "purities")
        engine._check(L.qk_bond_spectra_host(gpu_ctx._h, s.handle, 4, out.ctypes.data, None), "spectra")  # norms may be NULL
        assert np.abs(out.sum(-1) - 1.0).max() < 1e-12


# ---- 6. build_entanglement_profile --------------------------------------------------------------------------------------
def _profile_case():
    n = 8
    return Q.KernelStateAnsatz(n, 3, 1.0, Q.entanglement_graph(n, 2)), R.synthetic_features(7, n, 31)


def _exact_spectra(ans, x):
    circ = ans.circuit_for_data(x)
    psi = R.statevector(circ.n_qubits, [(name, tuple(qs), (p[0] if p else None)) for name, qs, p in circ.as_tuples()])
    return dense_spectra(psi, circ.n_qubits)


def test_build_entanglement_profile_both_builders(gpu_ctx, monkeypatch, tmp_path):
    import json

    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_entanglement_profile

    ans, X = _profile_case()
    exact = [_exact_spectra(ans, x) for x in X]
    got = {}
    for builder in ("host", "device"):
        monkeypatch.setenv("QK_BUILDER", builder)
        info = str(tmp_path / f"prof_{builder}")
        out = build_entanglement_profile(SingleComm(), ans, X, truncation_error=1e-16, info_file=info)
        S = out["spectra"]
        assert S.shape[:2] == (7, 7) and S.shape[2] == out["bond_dims"][:, 1:-1].max() and out["purities"].shape == (7, 7)
        assert out["norms"].shape == (7,) and np.abs(out["norms"] - 1.0).max() < 1e-10 and out["bond_dims"].shape == (7, 9)
        err = max(float(np.abs(S[i, k, : len(w)] - w[: S.shape[2]]).max()) for i, ex in enumerate(exact) for k, w in enumerate(ex))
        err_p = max(abs(out["purities"][i, k] - float((w * w).sum())) for i, ex in enumerate(exact) for k, w in enumerate(ex))
        print(f"build_entanglement_profile, {builder} builder: max |d lambda| vs exact state vectors = {err:.3e}, max |d purity| = {err_p:.3e}")
        assert err < 1e-10 and err_p < 1e-10
        prof = json.load(open(info + ".json"))
        assert prof["pqk_bond_values"] == [S.shape[2], "weights"] and "pqk_entanglement_time" in prof and prof["lenX"] == [7, "entries"]
        got[builder] = out
    assert all(max(int((w >= 1e-3).sum()) for w in ex) >= 2 for ex in exact)  # every state is entangled across some bond
    m = min(got["host"]["spectra"].shape[2], got["device"]["spectra"].shape[2])
    assert np.abs(got["host"]["spectra"][..., :m] - got["device"]["spectra"][..., :m]).max() < 1e-10
    assert np.abs(got["host"]["purities"] - got["device"]["purities"]).max() < 1e-10
    monkeypatch.setenv("QK_BUILDER", "host")
    few = build_entanglement_profile(SingleComm(), ans, X, truncation_error=1e-16, max_values=3)
    assert np.array_equal(few["spectra"], got["host"]["spectra"][..., :3])
    with pytest.raises(ValueError, match="max_values"):
        build_entanglement_profile(SingleComm(), ans, X, truncation_error=1e-16, max_values=0)


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
        from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_entanglement_profile
        from test_gpu_entanglement import _profile_case as case_

        ans, X = case_()
        q.put((rank, build_entanglement_profile(TorchComm(), ans, X, truncation_error=1e-16)))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_match_one_rank_bitwise(built, monkeypatch):
    import torch.multiprocessing as mp

    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_entanglement_profile

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + ((os.getpid() + 1511) % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    monkeypatch.setenv("QK_BUILDER", "host")
    ans, X = _profile_case()
    one = build_entanglement_profile(SingleComm(), ans, X, truncation_error=1e-16)
    for r in range(2):  # every rank returns the whole profile
        for key in ("spectra", "purities", "norms", "bond_dims"):
            assert np.array_equal(res[r][key], one[key]), (r, key)
