"""Projected quantum kernel on the MI355X: the device local sweep (qk_local_paulis_host) against the numpy reference of
tests/test_projected_host.py and exact state vectors, on canonical and on general-gauge states, its bit-reproducibility, the
PQK Gram kernel, and build_projected_kernel_matrix with one and two ranks."""
import os
import sys

import numpy as np
import pytest

import qml_cutensornet_amd as Q
from helpers import gauge_set_300, gauge_sets, golden_mps_sets
from oracle import restatement as R
from test_projected_host import bloch_from_dense, ref_local_paulis, ref_projected_gram

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _device_features(ctx, states):
    with ctx.upload(states) as s:
        return ctx.local_paulis(s, norms=True)


def _check_against_reference(ctx, states, tol=1e-12):
    F, norms = _device_features(ctx, states)
    assert F.shape == (len(states), len(states[0]), 3)
    for m, f, nrm in zip(states, F, norms):
        fr, nr = ref_local_paulis(m.tensors)
        assert np.abs(f - fr).max() < tol
        assert abs(nrm - nr) < 1e-12 * nr
    return F, norms


def _exact_bloch(ans, x):
    circ = ans.circuit_for_data(x)
    psi = R.statevector(circ.n_qubits, [(name, tuple(qs), (p[0] if p else None)) for name, qs, p in circ.as_tuples()])
    return bloch_from_dense(psi, circ.n_qubits)[0]


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
    _check_against_reference(gpu_ctx, [Q.random_mps(1, [1, 1], rng) for _ in range(3)])
    _check_against_reference(gpu_ctx, [Q.random_mps(2, [1, 2, 1], rng) for _ in range(3)])


def _worst_against_reference(F, norms, states):
    """(max |dF|, max relative |d norm|) against the numpy reference on the same tensors."""
    refs = [ref_local_paulis(m.tensors) for m in states]
    return (max(float(np.abs(f - fr).max()) for f, (fr, _) in zip(F, refs)),
            max(abs(nrm - nr) / nr for nrm, (_, nr) in zip(norms, refs)))


@pytest.mark.parametrize("sets,alone", [(gauge_sets, 3), (gauge_set_300, 1)], ids=["20-sites", "bond-300"])
def test_general_gauge_twins(gpu_ctx, sets, alone):
    """States whose L_k and R_k are dense and complex at every bond (tests/test_gauge_inputs_host.py), bonds across 16, 48, 64, 128
    and up to 300: the twins against the reference on their own tensors, against their right-orthonormal originals on the device
    (the references of the two drift by <= 1e-13), and one twin alone against itself in the set, bit for bit.  Measured on the
    MI355X: max |dF| = 1.1e-15 (20 sites) and 5.6e-16 (bond 300) on the twins, 1.1e-15 and 4.5e-16 on the originals; twin against
    original 1.7e-15."""
    originals, twins = sets()
    Fo, no = _device_features(gpu_ctx, list(originals))
    with gpu_ctx.upload(list(twins)) as s:
        F, nrm = gpu_ctx.local_paulis(s, norms=True)
    (ef, en), (eo, _) = _worst_against_reference(F, nrm, twins), _worst_against_reference(Fo, no, originals)
    scale = np.array([3.7**2 if k % 2 else 1.0 for k in range(len(twins))])
    dF, dn = float(np.abs(F - Fo).max()), float(np.abs(nrm / scale / no - 1.0).max())
    print(f"general gauge, {len(twins)} states, bonds up to {max(m.max_bond() for m in twins)}: max |dF| vs reference = {ef:.3e} on the twins "
          f"({eo:.3e} on the originals), norms {en:.3e}; twin vs original on the device: |dF| = {dF:.3e}, norms {dn:.3e}")
    assert ef < 1e-12 and eo < 1e-12 and en < 1e-12
    assert dF < 1e-12 + 1e-13 and dn < 1e-12 + 1e-13
    F1, n1 = _device_features(gpu_ctx, [twins[alone]])
    assert np.array_equal(F1[0], F[alone]) and n1[0] == nrm[alone]


def test_product_states(gpu_ctx):
    n = 6
    states = []
    for a in (0.1, -0.7, 1.3):
        gates = [("Ry", [0], [a]), ("Rx", [1], [a]), ("H", [2], []), ("Ry", [4], [2 * a]), ("Rx", [5], [-a])]
        states.append(Q.simulate(Q.BoundCircuit.from_gates(n, gates), 1 - 1e-16))
    assert max(m.max_bond() for m in states) == 1
    F, _ = _check_against_reference(gpu_ctx, states)
    assert abs(F[0, 0, 0] - np.sin(np.pi * 0.1)) < 1e-12 and abs(F[0, 2, 0] - 1.0) < 1e-12


def test_unnormalised_state(gpu_ctx):
    rng = np.random.default_rng(9)
    m = Q.random_mps(9, [1, 2, 4, 8, 16, 12, 8, 4, 2, 1], rng)
    scaled = Q.MPS([t * (3.7 if k == 4 else 1.0) for k, t in enumerate(m.tensors)])
    F, norms = _device_features(gpu_ctx, [m, scaled])
    assert abs(norms[1] - 3.7**2 * norms[0]) < 1e-12 * norms[1]
    assert abs(norms[1] - ref_local_paulis(scaled.tensors)[1]) < 1e-12 * norms[1]
    assert np.abs(F[0] - F[1]).max() < 1e-12


def test_device_built_set_and_exact_state_vectors(gpu_ctx):
    n = 12
    ans = Q.KernelStateAnsatz(n, 2, 1.0, Q.entanglement_graph(n, 2))
    X = R.synthetic_features(6, n, 21)
    circs = [ans.circuit_for_data(x) for x in X]
    dset, _, _ = gpu_ctx.build_share(circs, 1 - 1e-16, max_bond=256)
    assert dset is not None
    with dset:
        Fd = gpu_ctx.local_paulis(dset)
    Fh, _ = _device_features(gpu_ctx, [Q.simulate(c, 1 - 1e-16) for c in circs])
    assert np.abs(Fd - Fh).max() < 1e-10
    for f, x in zip(Fd, X):
        assert np.abs(f - _exact_bloch(ans, x)).max() < 1e-10


def test_state_alone_vs_in_a_set_and_repeat_bit_identical(gpu_ctx):
    rng = np.random.default_rng(2)
    prof = [1, 2, 4, 8, 16, 32, 64, 100, 64, 32, 16, 8, 4, 2, 1]
    big = [Q.random_mps(14, prof if k % 3 else [min(c, 20) for c in prof], rng) for k in range(40)]
    alone, _ = _device_features(gpu_ctx, [big[17]])
    with gpu_ctx.upload(big) as s:
        F1 = gpu_ctx.local_paulis(s)
        F2 = gpu_ctx.local_paulis(s)
    assert np.array_equal(alone[0], F1[17])
    assert np.array_equal(F1, F2)


def test_complex64_set_is_rejected(gpu_ctx):
    from qml_cutensornet_amd import engine

    rng = np.random.default_rng(0)
    with gpu_ctx.upload([Q.random_mps(4, [1, 2, 4, 2, 1], rng)]) as s, s.to_f32() as s32:
        with pytest.raises(engine.QkError, match="complex64"):
            gpu_ctx.local_paulis(s32)


def test_projected_gram_kernel(gpu_ctx):
    rng = np.random.default_rng(5)
    states = [Q.random_mps(10, [1, 2, 4, 8, 16, 16, 8, 4, 2, 1, 1], rng) for _ in range(70)]
    F, _ = _device_features(gpu_ctx, states)
    K = gpu_ctx.projected_gram(F)
    assert K.shape == (70, 70)
    assert np.abs(K - ref_projected_gram(F, F, 0.1)).max() < 1e-13
    assert np.array_equal(K, K.T) and np.all(np.diag(K) == 1.0)
    Kr = gpu_ctx.projected_gram(F, F[:23], gamma=0.37)
    assert Kr.shape == (23, 70)
    assert np.abs(Kr - ref_projected_gram(F, F[:23], 0.37)).max() < 1e-13
    K2 = gpu_ctx.projected_gram(F, F[:23], gamma=0.74)
    assert np.all(np.abs(K2 - Kr**2) <= 1e-13 * np.abs(K2))


def _exact_pqk(ans, X, Y, g):
    fx = np.stack([_exact_bloch(ans, x) for x in X])
    fy = fx if Y is None else np.stack([_exact_bloch(ans, y) for y in Y])
    return ref_projected_gram(fx, fy, g)


@pytest.mark.parametrize("builder", ["device", "host"])
def test_build_projected_kernel_matrix_exact(gpu_ctx, monkeypatch, tmp_path, builder):
    import json

    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_projected_kernel_matrix

    monkeypatch.setenv("QK_BUILDER", builder)
    n = 12
    ans = Q.KernelStateAnsatz(n, 2, 1.0, Q.entanglement_graph(n, 2))
    X, Y = R.synthetic_features(7, n, 8), R.synthetic_features(4, n, 9)
    info = str(tmp_path / "prof")
    K = build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, info_file=info)
    assert K.shape == (7, 7) and np.abs(K - _exact_pqk(ans, X, None, 1.0 / n)).max() < 1e-10
    prof = json.load(open(info + ".json"))
    assert prof["pqk_gamma"][0] == 1.0 / n and "pqk_features_time" in prof and "kernel_mat_time" in prof
    Kt = build_projected_kernel_matrix(SingleComm(), ans, X, Y=Y, pqk_gamma=0.2, truncation_error=1e-16)
    assert Kt.shape == (4, 7) and np.abs(Kt - _exact_pqk(ans, X, Y, 0.2)).max() < 1e-10


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
        out = {"train": build_projected_kernel_matrix(comm, ans, X, truncation_error=1e-16),
               "test": build_projected_kernel_matrix(comm, ans, X, Y=Y, truncation_error=1e-16)}
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
    port = 29600 + ((os.getpid() + 997) % 2000)
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
    one = build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16)
    one_t = build_projected_kernel_matrix(SingleComm(), ans, X, Y=Y, truncation_error=1e-16)
    assert np.array_equal(res[0]["train"], one)
    assert np.array_equal(res[0]["test"], one_t)
