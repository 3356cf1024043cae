"""Two-qubit projected quantum kernel over pairs up to a chosen distance, on the MI355X: the device distance sweep
(qk_local_pair_paulis_dist_host) against the numpy reference of tests/test_projected_dist_host.py and exact state vectors, its
bit guarantees (the distance-1 block, the Bloch vectors and the norms are the neighbour call's bits; a state alone, in a set and
repeated), the Gram kernel, and build_projected_kernel_matrix(rdm=2, pair_distance=2) with one and two ranks.  Mirrors
tests/test_gpu_projected_pair.py case for case, with its tolerances."""
import os
import sys

import numpy as np
import pytest

import qml_cutensornet_amd as Q
from helpers import gauge_sets, golden_mps_sets
from oracle import restatement as R
from qml_cutensornet_amd import engine
from test_projected_dist_host import pair_dist_from_dense, pair_index, ref_pair_paulis_dist
from test_projected_pair_host import ref_pair_gram

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _n_pairs(n, D):
    return D * n - D * (D + 1) // 2


def _device_features(ctx, states, D):
    with ctx.upload(states) as s:
        return ctx.local_pair_paulis(s, norms=True, max_dist=D)


def _check_against_reference(ctx, states, D, tol=1e-12):
    n = len(states[0])
    T, norms = _device_features(ctx, states, D)
    assert T.shape == (len(states), _n_pairs(n, D), 4, 4)
    assert np.all(T[:, :, 0, 0] == 1.0)
    worst = np.zeros(D + 1)
    refs = [ref_pair_paulis_dist(m.tensors, D) for m in states]
    for t, (tr, _) in zip(T, refs):
        for d in range(1, D + 1):
            lo, hi = pair_index(n, d, 0), pair_index(n, d, 0) + n - d
            worst[d] = max(worst[d], float(np.abs(t[lo:hi] - tr[lo:hi]).max()))
    print(f"distance sweep vs numpy reference, D = {D}, {len(states)} states of {n} qubits: max |dT| per distance = "
          + ", ".join(f"d{d}: {worst[d]:.3e}" for d in range(1, D + 1)))
    for t, nrm, (tr, nr) in zip(T, norms, refs):
        assert np.abs(t - tr).max() < tol
        assert abs(nrm - nr) < 1e-12 * nr
    return T, norms


def _raw_dist(ctx, mps_set, D, singles=False, norms=False):
    """The C entry point itself, also at max_dist = 1 (the Python wrapper sends max_dist = 1 to the neighbour call)."""
    info = mps_set.info()
    ns, n = info["n_states"], info["n_sites"]
    T = np.zeros((ns, _n_pairs(n, D), 4, 4))
    F = np.zeros((ns, n, 3)) if singles else None
    nrm = np.zeros(ns) if norms else None
    engine._check(engine.lib().qk_local_pair_paulis_dist_host(ctx._h, mps_set.handle, D, T.ctypes.data, None if F is None else F.ctypes.data,
                                                              None if nrm is None else nrm.ctypes.data), "qk_local_pair_paulis_dist_host")
    return T, F, nrm


def _exact_pairs(ans, x, D):
    circ = ans.circuit_for_data(x)
    psi = R.statevector(circ.n_qubits, [(name, tuple(qs), (p[0] if p else None)) for name, qs, p in circ.as_tuples()])
    return pair_dist_from_dense(psi, circ.n_qubits, D)[0]


def test_golden_mps(gpu_ctx):
    xs, ys, _ = golden_mps_sets()
    states = [Q.MPS(t) for t in xs + ys]
    for D in (2, len(states[0]) - 1):
        _check_against_reference(gpu_ctx, states, D)


def test_host_built_bonds_across_tiles(gpu_ctx):
    ans = Q.KernelStateAnsatz(14, 4, 1.0, Q.entanglement_graph(14, 3))
    states = [Q.simulate(ans.circuit_for_data(x), 1 - 1e-16) for x in R.synthetic_features(4, 14, 3)]
    assert max(m.max_bond() for m in states) >= 64
    _check_against_reference(gpu_ctx, states, 3)


def test_ragged_random_up_to_300_and_short_chains(gpu_ctx):
    rng = np.random.default_rng(4)
    profs = [[1, 2, 4, 8, 16, 32, 64, 128, 200, 300, 150, 75, 38, 19, 10, 5, 3, 2, 1], [1, 2, 4, 8, 16, 29, 40, 33, 17, 9, 5, 3, 2, 1]]
    for prof in profs:
        _check_against_reference(gpu_ctx, [Q.random_mps(len(prof) - 1, prof, rng) for _ in range(2)], 4)
    for prof in ([1, 2, 1], [1, 1, 1]):  # two-site chains: D = 1 is the only distance, through the distance entry point
        states = [Q.random_mps(2, prof, rng) for _ in range(3)]
        with gpu_ctx.upload(states) as s:
            T, _, nrm = _raw_dist(gpu_ctx, s, 1, norms=True)
        for m, t, nr in zip(states, T, nrm):
            tr, nref = ref_pair_paulis_dist(m.tensors, 1)
            assert np.abs(t - tr).max() < 1e-12 and abs(nr - nref) < 1e-12 * nref


def test_general_gauge_twins(gpu_ctx):
    """Two twins of ``gauge_sets`` (dense complex L_k and R_k, bonds up to 128 and 65, the second scaled by 3.7) at max_dist = 3
    against the reference on their own tensors (seconds per state, hence two), against their originals on the device, and the
    distance-1 rows, the Bloch vectors and the norms against the neighbour calls on the twins, bit for bit.  Measured on the
    MI355X: max |dT| = 1.3e-15 on the twins (distance 3), 1.7e-15 twin against original."""
    D, n = 3, 20
    originals, twins = (list(s[:2]) for s in gauge_sets())
    T, nrm = _check_against_reference(gpu_ctx, twins, D)
    To, no = _device_features(gpu_ctx, originals, D)
    dT, dn = float(np.abs(T - To).max()), float(np.abs(nrm / np.array([1.0, 3.7**2]) / no - 1.0).max())
    print(f"general gauge, D = {D}: twin vs original on the device: |dT| = {dT:.3e}, norms {dn:.3e}")
    assert dT < 1e-12 + 1e-13 and dn < 1e-12 + 1e-13
    with gpu_ctx.upload(twins) as s:
        F, nrm1 = gpu_ctx.local_paulis(s, norms=True)
        Tn = gpu_ctx.local_pair_paulis(s)
        T3, F3, nrm3 = gpu_ctx.local_pair_paulis(s, singles=True, norms=True, max_dist=D)
    assert np.array_equal(T3, T) and np.array_equal(T3[:, : n - 1], Tn)
    assert np.array_equal(F3, F) and np.array_equal(nrm3, nrm1) and np.array_equal(nrm3, nrm)


def test_product_states(gpu_ctx):
    n, D = 6, 5
    states = []
    for a in (0.1, -0.7, 1.3):
        gates = [("Ry", [0], [a]), ("Rx", [1], [a]), ("H", [2], []), ("Ry", [4], [2 * a]), ("Rx", [5], [-a])]
        states.append(Q.simulate(Q.BoundCircuit.from_gates(n, gates), 1 - 1e-16))
    assert max(m.max_bond() for m in states) == 1
    with gpu_ctx.upload(states) as s:
        T, F = gpu_ctx.local_pair_paulis(s, singles=True, max_dist=D)
    for m, t in zip(states, T):
        assert np.abs(t - ref_pair_paulis_dist(m.tensors, D)[0]).max() < 1e-12
    # every pair of a product state, at every distance, is the outer product of the two Pauli vectors (1, F)
    P = np.concatenate([np.ones((len(states), n, 1)), F], axis=2)
    for row, (a, b) in enumerate(engine.pair_table(n, D)):
        assert np.abs(T[:, row] - P[:, a, :, None] * P[:, b, None, :]).max() < 1e-12
    # pair (0, 5) of the first state: Ry(a)|0> (x) Rx(-a)|0>, the outer product of (1, sin, 0, cos) and (1, 0, sin, cos)
    s_, c_ = np.sin(np.pi * 0.1), np.cos(np.pi * 0.1)
    assert np.abs(T[0, pair_index(n, 5, 0)] - np.outer([1.0, s_, 0.0, c_], [1.0, 0.0, s_, c_])).max() < 1e-12


def test_analytic_xxphase_on_qubits_0_and_2(gpu_ctx):
    a = 0.3
    m = Q.simulate(Q.BoundCircuit.from_gates(3, [("XXPhase", [0, 2], [a])]), 1 - 1e-16)
    T, _ = _check_against_reference(gpu_ctx, [m], 2)
    want = np.zeros((4, 4))
    want[0, 0] = want[3, 3] = 1.0
    want[1, 2] = want[2, 1] = -np.sin(np.pi * a)
    want[3, 0] = want[0, 3] = np.cos(np.pi * a)
    assert np.abs(T[0, pair_index(3, 2, 0)] - want).max() < 1e-12


def test_unnormalised_state(gpu_ctx):
    rng = np.random.default_rng(9)
    m = Q.random_mps(9, [1, 2, 4, 8, 16, 12, 8, 4, 2, 1], rng)
    scaled = Q.MPS([t * (3.7 if k == 4 else 1.0) for k, t in enumerate(m.tensors)])
    T, norms = _device_features(gpu_ctx, [m, scaled], 4)
    assert abs(norms[1] - 3.7**2 * norms[0]) < 1e-12 * norms[1]
    assert abs(norms[1] - ref_pair_paulis_dist(scaled.tensors, 4)[1]) < 1e-12 * norms[1]
    assert np.abs(T[0] - T[1]).max() < 1e-12


def test_device_built_set_and_exact_state_vectors(gpu_ctx):
    n, D = 12, 3
    ans = Q.KernelStateAnsatz(n, 2, 1.0, Q.entanglement_graph(n, 2))
    X = R.synthetic_features(6, n, 21)
    circs = [ans.circuit_for_data(x) for x in X]
    dset, _, _ = gpu_ctx.build_share(circs, 1 - 1e-16, max_bond=256)
    assert dset is not None
    with dset:
        Td = gpu_ctx.local_pair_paulis(dset, max_dist=D)
    Th, _ = _device_features(gpu_ctx, [Q.simulate(c, 1 - 1e-16) for c in circs], D)
    assert np.abs(Td - Th).max() < 1e-10
    worst = 0.0
    for t, x in zip(Td, X):
        worst = max(worst, float(np.abs(t - _exact_pairs(ans, x, D)).max()))
    print(f"device-built set vs exact state vectors, D = {D}: max |dT| = {worst:.3e}")
    assert worst < 1e-10


def test_state_alone_vs_in_a_set_and_repeat_bit_identical(gpu_ctx):
    rng = np.random.default_rng(2)
    prof = [1, 2, 4, 8, 16, 32, 64, 100, 64, 32, 16, 8, 4, 2, 1]
    big = [Q.random_mps(14, prof if k % 3 else [min(c, 20) for c in prof], rng) for k in range(40)]
    alone, _ = _device_features(gpu_ctx, [big[17]], 3)
    with gpu_ctx.upload(big) as s:
        T1 = gpu_ctx.local_pair_paulis(s, max_dist=3)
        T2 = gpu_ctx.local_pair_paulis(s, max_dist=3)
    assert np.array_equal(alone[0], T1[17])
    assert np.array_equal(T1, T2)
    assert np.all(T1[:, :, 0, 0] == 1.0)


def test_distance_one_block_singles_and_norms_are_the_neighbour_calls_bits(gpu_ctx):
    rng = np.random.default_rng(12)
    prof = [1, 2, 4, 8, 16, 32, 64, 100, 64, 32, 16, 8, 4, 2, 1]
    n = 14
    states = [Q.random_mps(n, prof if k % 2 else [min(c, 24) for c in prof], rng) for k in range(9)]
    with gpu_ctx.upload(states) as s:
        F, nrm = gpu_ctx.local_paulis(s, norms=True)
        Tn = gpu_ctx.local_pair_paulis(s)
        for D in (1, 2, 4, n - 1):
            T, F2, nrm2 = _raw_dist(gpu_ctx, s, D, singles=True, norms=True)
            assert np.array_equal(T[:, : n - 1], Tn), D  # the distance-1 block, for any max_dist
            assert np.array_equal(F2, F) and np.array_equal(nrm2, nrm), D
            if D == 1:
                assert np.array_equal(T, Tn)
            else:
                T3, F3 = gpu_ctx.local_pair_paulis(s, singles=True, max_dist=D)
                assert np.array_equal(T3, T) and np.array_equal(F3, F)
                assert np.array_equal(gpu_ctx.local_pair_paulis(s, max_dist=D), T)
        T4 = _raw_dist(gpu_ctx, s, 4)[0]
    # a smaller max_dist is a prefix of a larger one
    assert np.array_equal(T4[:, : _n_pairs(n, 2)], _raw_dist_prefix(gpu_ctx, states, 2))
    # the margins of every pair are the Bloch vectors, to rounding
    for row, (a, b) in enumerate(engine.pair_table(n, 4)):
        assert np.abs(T4[:, row, 1:, 0] - F[:, a]).max() < 1e-12
        assert np.abs(T4[:, row, 0, 1:] - F[:, b]).max() < 1e-12


def _raw_dist_prefix(ctx, states, D):
    with ctx.upload(states) as s:
        return _raw_dist(ctx, s, D)[0]


def test_bad_max_dist_complex64_and_one_site_sets_are_rejected(gpu_ctx):
    rng = np.random.default_rng(0)
    with gpu_ctx.upload([Q.random_mps(4, [1, 2, 4, 2, 1], rng)]) as s, s.to_f32() as s32:
        for bad in (0, 4, -1):  # max_dist = 0 and max_dist = n
            with pytest.raises(engine.QkError, match="max_dist"):
                gpu_ctx.local_pair_paulis(s, max_dist=bad)
        with pytest.raises(engine.QkError, match="complex64"):
            gpu_ctx.local_pair_paulis(s32, max_dist=2)
    with gpu_ctx.upload([Q.random_mps(1, [1, 1], rng)]) as s1:
        with pytest.raises(engine.QkError, match="n_sites"):
            gpu_ctx.local_pair_paulis(s1, max_dist=2)
    t = np.zeros((2, 5, 4, 4))
    out = np.zeros((2, 2))
    L = engine.lib()
    for bad in (0, 4):
        with pytest.raises(engine.QkError, match="max_dist"):
            engine._check(L.qk_projected_pair_gram_dist_host(gpu_ctx._h, 4, bad, 2, t.ctypes.data, 2, None, 0.5, out.ctypes.data, 2), "gram")
    with pytest.raises(engine.QkError, match="g must be"):
        engine._check(L.qk_projected_pair_gram_dist_host(gpu_ctx._h, 4, 2, 2, t.ctypes.data, 2, None, 0.0, out.ctypes.data, 2), "gram")
    with pytest.raises(engine.QkError, match="n_sites"):
        engine._check(L.qk_projected_pair_gram_dist_host(gpu_ctx._h, 1, 1, 2, t.ctypes.data, 2, None, 0.5, out.ctypes.data, 2), "gram")


def test_projected_pair_gram_dist_kernel(gpu_ctx):
    rng = np.random.default_rng(5)
    n, D = 10, 3
    states = [Q.random_mps(n, [1, 2, 4, 8, 16, 16, 8, 4, 2, 1, 1], rng) for _ in range(70)]
    T, _ = _device_features(gpu_ctx, states, D)
    K = gpu_ctx.projected_pair_gram(T, max_dist=D)
    assert K.shape == (70, 70)
    assert np.abs(K - ref_pair_gram(T, T, 1.0 / (n * D))).max() < 1e-13  # the default bandwidth 1 / (n_qubits D)
    assert np.array_equal(K, K.T) and np.all(np.diag(K) == 1.0)
    Kr = gpu_ctx.projected_pair_gram(T, T[:23], gamma=0.37, max_dist=D)
    assert Kr.shape == (23, 70)
    assert np.abs(Kr - ref_pair_gram(T, T[:23], 0.37)).max() < 1e-13
    K2 = gpu_ctx.projected_pair_gram(T, T[:23], gamma=0.74, max_dist=D)
    assert np.all(np.abs(K2 - Kr**2) <= 1e-13 * np.abs(K2))
    # max_dist = 1 through the distance entry point is the neighbour Gram, bit for bit
    T1 = np.ascontiguousarray(T[:, : n - 1])
    Kn = gpu_ctx.projected_pair_gram(T1, T1[:23], gamma=0.37)
    Kd = np.zeros_like(Kn)
    engine._check(engine.lib().qk_projected_pair_gram_dist_host(gpu_ctx._h, n, 1, 70, T1.ctypes.data, 23, T1[:23].ctypes.data, 0.37, Kd.ctypes.data, 70),
                  "qk_projected_pair_gram_dist_host")
    assert np.array_equal(Kd, Kn)


def _exact_pqk2(ans, X, Y, g, D):
    tx = np.stack([_exact_pairs(ans, x, D) for x in X])
    ty = tx if Y is None else np.stack([_exact_pairs(ans, y, D) for y in Y])
    return ref_pair_gram(tx, ty, g)


@pytest.mark.parametrize("builder", ["device", "host"])
def test_build_projected_kernel_matrix_pair_distance_exact(gpu_ctx, monkeypatch, tmp_path, builder):
    import json

    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_projected_kernel_matrix

    monkeypatch.setenv("QK_BUILDER", builder)
    n, D = 12, 2
    ans = Q.KernelStateAnsatz(n, 2, 1.0, Q.entanglement_graph(n, 2))
    X, Y = R.synthetic_features(7, n, 8), R.synthetic_features(4, n, 9)
    info = str(tmp_path / "prof")
    K = build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, info_file=info, rdm=2, pair_distance=D)
    err = float(np.abs(K - _exact_pqk2(ans, X, None, 1.0 / (n * D), D)).max())
    print(f"build_projected_kernel_matrix(rdm=2, pair_distance={D}), {builder} builder: max |dK| = {err:.3e}")
    assert K.shape == (7, 7) and err < 1e-10
    prof = json.load(open(info + ".json"))
    assert prof["pqk_rdm"][0] == 2 and prof["pqk_pair_distance"] == [D, "sites"]
    assert prof["pqk_gamma"][0] == 1.0 / (n * D) and "pqk_features_time" in prof and "kernel_mat_time" in prof
    Kt = build_projected_kernel_matrix(SingleComm(), ans, X, Y=Y, pqk_gamma=0.2, truncation_error=1e-16, rdm=2, pair_distance=D)
    assert Kt.shape == (4, 7) and np.abs(Kt - _exact_pqk2(ans, X, Y, 0.2, D)).max() < 1e-10
    # the neighbour form of the same call is a different matrix, also at the same bandwidth: the distance-2 pairs carry signal
    K1 = build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, info_file=info, rdm=2, pair_distance=1)
    assert json.load(open(info + ".json"))["pqk_pair_distance"] == [1, "sites"]
    assert np.abs(K1 - K).max() > 1e-3
    K1g = build_projected_kernel_matrix(SingleComm(), ans, X, pqk_gamma=1.0 / (n * D), truncation_error=1e-16, rdm=2)
    assert np.abs(K1g - K).max() > 1e-3
    # the one-qubit form has no such key
    build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, info_file=info, rdm=1)
    assert "pqk_pair_distance" not in json.load(open(info + ".json"))


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
        out = {"train": build_projected_kernel_matrix(comm, ans, X, truncation_error=1e-16, rdm=2, pair_distance=2),
               "test": build_projected_kernel_matrix(comm, ans, X, Y=Y, truncation_error=1e-16, rdm=2, pair_distance=2)}
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
    port = 29600 + ((os.getpid() + 1731) % 2000)
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
    one = build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, rdm=2, pair_distance=2)
    one_t = build_projected_kernel_matrix(SingleComm(), ans, X, Y=Y, truncation_error=1e-16, rdm=2, pair_distance=2)
    assert np.array_equal(res[0]["train"], one)
    assert np.array_equal(res[0]["test"], one_t)
