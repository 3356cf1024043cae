"""Two-qubit projected quantum kernel on the MI355X: the device pair sweep (qk_local_pair_paulis_host) against the numpy
reference of tests/test_projected_pair_host.py and exact state vectors, its bit-reproducibility and its agreement with the
one-qubit sweep, the pair Gram kernel, and build_projected_kernel_matrix(rdm=2) with one and two ranks.  Mirrors
tests/test_gpu_projected.py case for case, with its tolerances."""
import os
import sys

import numpy as np
import pytest

import qml_cutensornet_amd as Q
from helpers import gauge_set_300, gauge_sets, golden_mps_sets
from oracle import restatement as R
from test_projected_pair_host import pair_from_dense, ref_pair_gram, ref_pair_paulis

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _device_features(ctx, states):
    with ctx.upload(states) as s:
        return ctx.local_pair_paulis(s, norms=True)


def _check_against_reference(ctx, states, tol=1e-12):
    T, norms = _device_features(ctx, states)
    assert T.shape == (len(states), len(states[0]) - 1, 4, 4)
    assert np.all(T[:, :, 0, 0] == 1.0)
    worst = 0.0
    for m, t, nrm in zip(states, T, norms):
        tr, nr = ref_pair_paulis(m.tensors)
        worst = max(worst, float(np.abs(t - tr).max()))
        assert np.abs(t - tr).max() < tol
        assert abs(nrm - nr) < 1e-12 * nr
    print(f"pair sweep vs numpy reference: max |dT| = {worst:.3e} over {len(states)} states")
    return T, norms


def _exact_pairs(ans, x):
    circ = ans.circuit_for_data(x)
    psi = R.statevector(circ.n_qubits, [(name, tuple(qs), (p[0] if p else None)) for name, qs, p in circ.as_tuples()])
    return pair_from_dense(psi, circ.n_qubits)[0]


def test_golden_mps(gpu_ctx):
    xs, ys, _ = golden_mps_sets()
    _check_against_reference(gpu_ctx, [Q.MPS(t) for t in xs + ys])


def test_host_built_bonds_across_tiles(gpu_ctx):
    ans = Q.KernelStateAnsatz(14, 4, 1.0, Q.entanglement_graph(14, 3))
    states = [Q.simulate(ans.circuit_for_data(x), 1 - 1e-16) for x in R.synthetic_features(4, 14, 3)]
    assert max(m.max_bond() for m in states) >= 64
    _check_against_reference(gpu_ctx, states)


def test_ragged_random_up_to_300_and_short_chains(gpu_ctx):
    rng = np.random.default_rng(4)
    profs = [[1, 2, 4, 8, 16, 32, 64, 128, 200, 300, 150, 75, 38, 19, 10, 5, 3, 2, 1], [1, 2, 4, 8, 16, 29, 40, 33, 17, 9, 5, 3, 2, 1]]
    for prof in profs:
        _check_against_reference(gpu_ctx, [Q.random_mps(len(prof) - 1, prof, rng) for _ in range(2)])
    _check_against_reference(gpu_ctx, [Q.random_mps(2, [1, 2, 1], rng) for _ in range(3)])
    _check_against_reference(gpu_ctx, [Q.random_mps(2, [1, 1, 1], rng) for _ in range(3)])


def _worst_against_reference(T, norms, states):
    """(max |dT|, max relative |d norm|) against the numpy reference on the same tensors."""
    refs = [ref_pair_paulis(m.tensors) for m in states]
    return (max(float(np.abs(t - tr).max()) for t, (tr, _) in zip(T, refs)),
            max(abs(nrm - nr) / nr for nrm, (_, nr) in zip(norms, refs)))


@pytest.mark.parametrize("sets,alone", [(gauge_sets, 3), (gauge_set_300, 1)], ids=["20-sites", "bond-300"])
def test_general_gauge_twins(gpu_ctx, sets, alone):
    """The case of tests/test_gpu_projected.py for the pair sweep: twins with dense complex L_k and R_k against the reference on
    their own tensors, against their originals on the device, one twin alone against itself in the set.  Measured on the MI355X:
    max |dT| = 1.0e-15 (20 sites) and 7.8e-16 (bond 300) on the twins, 1.0e-15 and 5.5e-16 on the originals; twin against original
    1.7e-15."""
    originals, twins = sets()
    To, no = _device_features(gpu_ctx, list(originals))
    with gpu_ctx.upload(list(twins)) as s:
        T, nrm = gpu_ctx.local_pair_paulis(s, norms=True)
    (et, en), (eo, _) = _worst_against_reference(T, nrm, twins), _worst_against_reference(To, no, originals)
    scale = np.array([3.7**2 if k % 2 else 1.0 for k in range(len(twins))])
    dT, dn = float(np.abs(T - To).max()), float(np.abs(nrm / scale / no - 1.0).max())
    print(f"general gauge, {len(twins)} states, bonds up to {max(m.max_bond() for m in twins)}: max |dT| vs reference = {et:.3e} on the twins "
          f"({eo:.3e} on the originals), norms {en:.3e}; twin vs original on the device: |dT| = {dT:.3e}, norms {dn:.3e}")
    assert np.all(T[:, :, 0, 0] == 1.0)
    assert et < 1e-12 and eo < 1e-12 and en < 1e-12
    assert dT < 1e-12 + 1e-13 and dn < 1e-12 + 1e-13
    T1, n1 = _device_features(gpu_ctx, [twins[alone]])
    assert np.array_equal(T1[0], T[alone]) and n1[0] == nrm[alone]


def test_product_states(gpu_ctx):
    n = 6
    states = []
    for a in (0.1, -0.7, 1.3):
        gates = [("Ry", [0], [a]), ("Rx", [1], [a]), ("H", [2], []), ("Ry", [4], [2 * a]), ("Rx", [5], [-a])]
        states.append(Q.simulate(Q.BoundCircuit.from_gates(n, gates), 1 - 1e-16))
    assert max(m.max_bond() for m in states) == 1
    T, _ = _check_against_reference(gpu_ctx, states)
    # pair (0, 1) of the first state: Ry(a)|0> (x) Rx(a)|0>, the outer product of (1, sin, 0, cos) and (1, 0, -sin, cos)
    s, c = np.sin(np.pi * 0.1), np.cos(np.pi * 0.1)
    assert np.abs(T[0, 0] - np.outer([1.0, s, 0.0, c], [1.0, 0.0, -s, c])).max() < 1e-12
    assert abs(T[0, 1, 0, 1] - 1.0) < 1e-12  # <I X> of pair (1, 2): qubit 2 is H|0>


def test_analytic_xxphase_pair(gpu_ctx):
    a = 0.3
    m = Q.simulate(Q.BoundCircuit.from_gates(3, [("XXPhase", [0, 1], [a]), ("Ry", [2], [0.25])]), 1 - 1e-16)
    T, _ = _check_against_reference(gpu_ctx, [m])
    want = np.zeros((4, 4))
    want[0, 0] = want[3, 3] = 1.0
    want[1, 2] = want[2, 1] = -np.sin(np.pi * a)
    want[3, 0] = want[0, 3] = np.cos(np.pi * a)
    assert np.abs(T[0, 0] - want).max() < 1e-12


def test_unnormalised_state(gpu_ctx):
    rng = np.random.default_rng(9)
    m = Q.random_mps(9, [1, 2, 4, 8, 16, 12, 8, 4, 2, 1], rng)
    scaled = Q.MPS([t * (3.7 if k == 4 else 1.0) for k, t in enumerate(m.tensors)])
    T, norms = _device_features(gpu_ctx, [m, scaled])
    assert abs(norms[1] - 3.7**2 * norms[0]) < 1e-12 * norms[1]
    assert abs(norms[1] - ref_pair_paulis(scaled.tensors)[1]) < 1e-12 * norms[1]
    assert np.abs(T[0] - T[1]).max() < 1e-12


def test_device_built_set_and_exact_state_vectors(gpu_ctx):
    n = 12
    ans = Q.KernelStateAnsatz(n, 2, 1.0, Q.entanglement_graph(n, 2))
    X = R.synthetic_features(6, n, 21)
    circs = [ans.circuit_for_data(x) for x in X]
    dset, _, _ = gpu_ctx.build_share(circs, 1 - 1e-16, max_bond=256)
    assert dset is not None
    with dset:
        Td = gpu_ctx.local_pair_paulis(dset)
    Th, _ = _device_features(gpu_ctx, [Q.simulate(c, 1 - 1e-16) for c in circs])
    assert np.abs(Td - Th).max() < 1e-10
    for t, x in zip(Td, X):
        assert np.abs(t - _exact_pairs(ans, x)).max() < 1e-10


def test_state_alone_vs_in_a_set_and_repeat_bit_identical(gpu_ctx):
    rng = np.random.default_rng(2)
    prof = [1, 2, 4, 8, 16, 32, 64, 100, 64, 32, 16, 8, 4, 2, 1]
    big = [Q.random_mps(14, prof if k % 3 else [min(c, 20) for c in prof], rng) for k in range(40)]
    alone, _ = _device_features(gpu_ctx, [big[17]])
    with gpu_ctx.upload(big) as s:
        T1 = gpu_ctx.local_pair_paulis(s)
        T2 = gpu_ctx.local_pair_paulis(s)
    assert np.array_equal(alone[0], T1[17])
    assert np.array_equal(T1, T2)


def test_singles_and_norms_are_the_one_qubit_sweeps_bits(gpu_ctx):
    rng = np.random.default_rng(12)
    prof = [1, 2, 4, 8, 16, 32, 64, 100, 64, 32, 16, 8, 4, 2, 1]
    states = [Q.random_mps(14, prof if k % 2 else [min(c, 24) for c in prof], rng) for k in range(9)]
    with gpu_ctx.upload(states) as s:
        F, nrm = gpu_ctx.local_paulis(s, norms=True)
        T, F2, nrm2 = gpu_ctx.local_pair_paulis(s, singles=True, norms=True)
        T3, F3 = gpu_ctx.local_pair_paulis(s, singles=True)
        T4 = gpu_ctx.local_pair_paulis(s)
    assert np.array_equal(F2, F) and np.array_equal(nrm2, nrm) and np.array_equal(F3, F)
    assert np.array_equal(T3, T) and np.array_equal(T4, T)
    # the margins of T are the Bloch vectors, to rounding: T[k][p][0] = F[k][p-1], T[k][0][q] = F[k+1][q-1]
    assert np.abs(T[:, :, 1:, 0] - F[:, :-1]).max() < 1e-12
    assert np.abs(T[:, :, 0, 1:] - F[:, 1:]).max() < 1e-12


def test_complex64_and_one_site_sets_are_rejected(gpu_ctx):
    from qml_cutensornet_amd import engine

    rng = np.random.default_rng(0)
    with gpu_ctx.upload([Q.random_mps(4, [1, 2, 4, 2, 1], rng)]) as s, s.to_f32() as s32:
        with pytest.raises(engine.QkError, match="complex64"):
            gpu_ctx.local_pair_paulis(s32)
    with gpu_ctx.upload([Q.random_mps(1, [1, 1], rng)]) as s1:
        with pytest.raises(engine.QkError, match="n_sites"):
            gpu_ctx.local_pair_paulis(s1)
    with pytest.raises(engine.QkError, match="g must be"):
        _raw_gram_bad_g(gpu_ctx)


def _raw_gram_bad_g(ctx):
    """The C entry point's own check of g (the Python wrapper rejects a bad gamma before the call)."""
    from qml_cutensornet_amd import engine

    t = np.zeros((2, 3, 4, 4))
    out = np.zeros((2, 2))
    engine._check(engine.lib().qk_projected_pair_gram_host(ctx._h, 4, 2, t.ctypes.data, 2, None, 0.0, out.ctypes.data, 2), "qk_projected_pair_gram_host")


def test_projected_pair_gram_kernel(gpu_ctx):
    rng = np.random.default_rng(5)
    states = [Q.random_mps(10, [1, 2, 4, 8, 16, 16, 8, 4, 2, 1, 1], rng) for _ in range(70)]
    T, _ = _device_features(gpu_ctx, states)
    K = gpu_ctx.projected_pair_gram(T)
    assert K.shape == (70, 70)
    assert np.abs(K - ref_pair_gram(T, T, 0.1)).max() < 1e-13
    assert np.array_equal(K, K.T) and np.all(np.diag(K) == 1.0)
    Kr = gpu_ctx.projected_pair_gram(T, T[:23], gamma=0.37)
    assert Kr.shape == (23, 70)
    assert np.abs(Kr - ref_pair_gram(T, T[:23], 0.37)).max() < 1e-13
    K2 = gpu_ctx.projected_pair_gram(T, T[:23], gamma=0.74)
    assert np.all(np.abs(K2 - Kr**2) <= 1e-13 * np.abs(K2))


def _exact_pqk2(ans, X, Y, g):
    tx = np.stack([_exact_pairs(ans, x) for x in X])
    ty = tx if Y is None else np.stack([_exact_pairs(ans, y) for y in Y])
    return ref_pair_gram(tx, ty, g)


@pytest.mark.parametrize("builder", ["device", "host"])
def test_build_projected_kernel_matrix_rdm2_exact(gpu_ctx, monkeypatch, tmp_path, builder):
    import json

    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_projected_kernel_matrix

    monkeypatch.setenv("QK_BUILDER", builder)
    n = 12
    ans = Q.KernelStateAnsatz(n, 2, 1.0, Q.entanglement_graph(n, 2))
    X, Y = R.synthetic_features(7, n, 8), R.synthetic_features(4, n, 9)
    info = str(tmp_path / "prof")
    K = build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, info_file=info, rdm=2)
    assert K.shape == (7, 7) and np.abs(K - _exact_pqk2(ans, X, None, 1.0 / n)).max() < 1e-10
    prof = json.load(open(info + ".json"))
    assert prof["pqk_rdm"][0] == 2
    assert prof["pqk_gamma"][0] == 1.0 / n and "pqk_features_time" in prof and "kernel_mat_time" in prof
    Kt = build_projected_kernel_matrix(SingleComm(), ans, X, Y=Y, pqk_gamma=0.2, truncation_error=1e-16, rdm=2)
    assert Kt.shape == (4, 7) and np.abs(Kt - _exact_pqk2(ans, X, Y, 0.2)).max() < 1e-10
    # the one-qubit form of the same call is a different matrix, and says so in its JSON
    K1 = build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, info_file=info, rdm=1)
    assert json.load(open(info + ".json"))["pqk_rdm"][0] == 1
    assert np.abs(K1 - K).max() > 1e-3


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["QK_BUILDER"] = "host"
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import qml_cutensornet_amd as Q_
        from oracle import restatement as R_
        from qml_cutensornet_amd.dist import TorchComm
        from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_projected_kernel_matrix

        n = 10
        ans = Q_.KernelStateAnsatz(n, 2, 1.0, Q_.entanglement_graph(n, 2))
        X, Y = R_.synthetic_features(9, n, 13), R_.synthetic_features(5, n, 14)
        comm = TorchComm()
        out = {"train": build_projected_kernel_matrix(comm, ans, X, truncation_error=1e-16, rdm=2),
               "test": build_projected_kernel_matrix(comm, ans, X, Y=Y, truncation_error=1e-16, rdm=2)}
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_match_one_rank_bitwise(built, monkeypatch):
    import torch.multiprocessing as mp

    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_projected_kernel_matrix

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + ((os.getpid() + 1499) % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert res[1]["train"] is None and res[1]["test"] is None
    monkeypatch.setenv("QK_BUILDER", "host")
    n = 10
    ans = Q.KernelStateAnsatz(n, 2, 1.0, Q.entanglement_graph(n, 2))
    X, Y = R.synthetic_features(9, n, 13), R.synthetic_features(5, n, 14)
    one = build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, rdm=2)
    one_t = build_projected_kernel_matrix(SingleComm(), ans, X, Y=Y, truncation_error=1e-16, rdm=2)
    assert np.array_equal(res[0]["train"], one)
    assert np.array_equal(res[0]["test"], one_t)
