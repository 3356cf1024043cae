"""Pauli-string expectation values and the Gram over them, on the MI355X: qk_pauli_strings_host against the numpy reference of
tests/test_pauli_strings_host.py, exact state vectors and the merged device forms (Bloch vectors, pair correlators up to a
distance), its bit guarantees (a state alone, repeated, the strings reordered, one string alone, the batches cut by
QK_STRINGS_BATCH), the rejections, qk_feature_gram_host, and build_projected_kernel_matrix(observables=...) with one and two
ranks.  The tolerances are those of the merged projected-kernel tests.

Random full-weight strings are numerically zero on these states, so a comparison uses sparse strings (weight 1..4 inside a window
of 6 sites) and asserts that at least half of its reference values are >= 1e-3 in magnitude."""
import os
import sys

import numpy as np
import pytest

import qml_cutensornet_amd as Q
from helpers import gauge_set_300, gauge_sets, golden_mps_sets
from oracle import restatement as R
from qml_cutensornet_amd import engine
from test_pauli_strings_host import pair_strings, pauli_strings_from_dense, ref_pauli_strings, sparse_strings, weight_one_strings
from test_projected_host import ref_local_paulis

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case_strings(n, rng, count=60):
    """The string list of a comparison: sparse strings, then supports that start at site 0, end at site n - 1, a single site,
    identity gaps inside a support, full-length strings, the all-identity string and a duplicate."""
    S = [sparse_strings(n, count, rng)]
    extra = np.zeros((8, n), dtype=np.uint8)
    extra[0, 0] = 3                                  # single site, starts at 0
    extra[1, n - 1] = 1                              # single site, ends at n - 1
    extra[2, n // 2] = 2                             # single site inside
    extra[3, 0], extra[3, min(2, n - 1)] = 3, 3      # starts at 0, an identity gap
    extra[4, max(0, n - 4)], extra[4, n - 1] = 1, 1  # ends at n - 1, identity gaps
    extra[5, 0], extra[5, n - 1] = 3, 3              # the whole chain as support, identity inside
    extra[6] = 3                                     # full length
    extra[7] = rng.integers(1, 4, size=n)            # full length, random codes
    S.append(extra)
    S.append(np.zeros((1, n), dtype=np.uint8))       # all identity
    S.append(S[0][:1])                               # a duplicate of the first string
    return np.ascontiguousarray(np.vstack(S))


def _device_values(ctx, states, S):
    with ctx.upload(states) as s:
        return ctx.pauli_expectations(s, S, norms=True)


def _check_against_reference(ctx, states, S, tol=1e-12, label=""):
    V, norms = _device_values(ctx, states, S)
    assert V.shape == (len(states), len(S)) and V.dtype == np.float64
    refs = [ref_pauli_strings(m.tensors, S) for m in states]
    ref = np.stack([r[0] for r in refs])
    share = float((np.abs(ref) >= 1e-3).mean())
    err = float(np.abs(V - ref).max())
    print(f"pauli strings vs numpy reference {label}: {len(states)} states x {len(S)} strings, max |dV| = {err:.3e}, "
          f"share of |ref| >= 1e-3: {share:.2f}")
    assert share >= 0.5
    assert err < tol
    for nrm, (_, nr) in zip(norms, refs):
        assert abs(nrm - nr) < 1e-12 * nr
    ident = np.flatnonzero(~S.any(axis=1))
    assert ident.size and np.all(V[:, ident] == 1.0)
    assert np.array_equal(V[:, -1], V[:, 0])  # the duplicate
    return V, norms


# ---- 1. against the numpy reference ---------------------------------------------------------------------------------
def test_golden_mps(gpu_ctx):
    xs, ys, _ = golden_mps_sets()
    states = [Q.MPS(t) for t in xs + ys]
    _check_against_reference(gpu_ctx, states, case_strings(len(states[0]), np.random.default_rng(1)), label="(golden sets)")


@pytest.mark.parametrize("prof", [[1, 2, 4, 8, 16, 32, 64, 128, 200, 300, 150, 75, 38, 19, 10, 5, 3, 2, 1], [1, 2, 4, 8, 16, 29, 40, 33, 17, 9, 5, 3, 2, 1]],
                         ids=["bond300", "bond40"])
def test_ragged_random(gpu_ctx, prof):
    rng = np.random.default_rng(4)
    n = len(prof) - 1
    _check_against_reference(gpu_ctx, [Q.random_mps(n, prof, rng) for _ in range(2)], case_strings(n, rng), label=f"(random, bonds up to {max(prof)})")


def test_host_built_bonds_across_tiles(gpu_ctx):
    ans = Q.KernelStateAnsatz(14, 4, 1.0, Q.entanglement_graph(14, 3))
    states = [Q.simulate(ans.circuit_for_data(x), 1 - 1e-16) for x in R.synthetic_features(4, 14, 3)]
    assert max(m.max_bond() for m in states) >= 64
    _check_against_reference(gpu_ctx, states, case_strings(14, np.random.default_rng(6)), label="(host-built, 14 qubits)")


@pytest.mark.parametrize("sets,seed", [(gauge_sets, 135), (gauge_set_300, 300)], ids=["20-sites", "bond-300"])
def test_general_gauge_twins(gpu_ctx, sets, seed):
    """Twins with dense complex L_k and R_k at every bond (tests/test_gauge_inputs_host.py) against the reference on their own
    tensors, and against their right-orthonormal originals on the device (the references of the two drift by <= 1e-13).
    Measured on the MI355X: max |dV| = 7.8e-16 (20 sites) and 2.8e-16 (bond 300) on the twins, 5.6e-16 and 2.8e-16 on the originals;
    twin against original 1.0e-15."""
    originals, twins = sets()
    n = len(twins[0])
    S = case_strings(n, np.random.default_rng(seed))
    V, nrm = _check_against_reference(gpu_ctx, list(twins), S, label=f"(general gauge, bonds up to {max(m.max_bond() for m in twins)})")
    Vo, no = _check_against_reference(gpu_ctx, list(originals), S, label="(their right-orthonormal originals)")
    scale = np.array([3.7**2 if k % 2 else 1.0 for k in range(len(twins))])
    dV, dn = float(np.abs(V - Vo).max()), float(np.abs(nrm / scale / no - 1.0).max())
    print(f"twin vs original on the device: |dV| = {dV:.3e}, norms {dn:.3e}")
    assert dV < 1e-12 + 1e-13 and dn < 1e-12 + 1e-13


# ---- 2. short chains ----------------------------------------------------------------------------------------------------
def test_short_chains(gpu_ctx):
    rng = np.random.default_rng(8)
    cases = [([1, 1], np.arange(4, dtype=np.uint8).reshape(4, 1))]
    two = np.array([[p, q] for p in range(4) for q in range(4)], dtype=np.uint8)
    cases += [([1, 2, 1], two), ([1, 1, 1], two)]
    for prof, S in cases:
        states = [Q.random_mps(len(prof) - 1, prof, rng) for _ in range(3)]
        V, norms = _device_values(gpu_ctx, states, S)
        for m, v, nrm in zip(states, V, norms):
            vr, nr = ref_pauli_strings(m.tensors, S)
            assert np.abs(v - vr).max() < 1e-12 and abs(nrm - nr) < 1e-12 * nr
        assert np.all(V[:, 0] == 1.0)


def test_product_states(gpu_ctx):
    n = 6
    states = []
    for a in (0.1, -0.7, 1.3):
        gates = [("Ry", [0], [a]), ("Rx", [1], [a]), ("H", [2], []), ("Ry", [3], [0.2]), ("Rx", [3], [0.6 * a]), ("Ry", [4], [2 * a]), ("Rx", [5], [-a])]
        states.append(Q.simulate(Q.BoundCircuit.from_gates(n, gates), 1 - 1e-16))
    assert max(m.max_bond() for m in states) == 1
    S = case_strings(n, np.random.default_rng(3))
    V, _ = _device_values(gpu_ctx, states, S)
    for m, v in zip(states, V):
        F = ref_local_paulis(m.tensors)[0]
        want = np.array([np.prod([F[k, c[k] - 1] for k in np.flatnonzero(c)]) for c in S])
        assert np.abs(v - want).max() < 1e-12
    # H|0> on qubit 2: <X_2> = 1
    assert np.abs(gpu_ctx_values_of(gpu_ctx, states, [("X", (2,))]) - 1.0).max() < 1e-12


def gpu_ctx_values_of(ctx, states, specs):
    with ctx.upload(states) as s:
        return ctx.pauli_expectations(s, specs)


def test_analytic_xxphase(gpu_ctx):
    a = 0.3
    m = Q.simulate(Q.BoundCircuit.from_gates(2, [("XXPhase", [0, 1], [a])]), 1 - 1e-16)
    v = gpu_ctx_values_of(gpu_ctx, [m], ["XY", "YX", "ZZ", "XX", "II"])[0]
    assert np.abs(v - [-np.sin(np.pi * a), -np.sin(np.pi * a), 1.0, 0.0, 1.0]).max() < 1e-12


# ---- 3. against the merged device forms ---------------------------------------------------------------------------------
def test_against_local_paulis_and_pair_correlators_on_one_set(gpu_ctx):
    rng = np.random.default_rng(12)
    prof = [1, 2, 4, 8, 16, 32, 64, 100, 64, 32, 16, 8, 4, 2, 1]
    n, D = 14, 3
    states = [Q.random_mps(n, prof if k % 2 else [min(c, 24) for c in prof], rng) for k in range(9)]
    with gpu_ctx.upload(states) as s:
        F, nrm = gpu_ctx.local_paulis(s, norms=True)
        T = gpu_ctx.local_pair_paulis(s, max_dist=D)
        V1, nrm1 = gpu_ctx.pauli_expectations(s, weight_one_strings(n), norms=True)
        V2, nrm2 = gpu_ctx.pauli_expectations(s, pair_strings(n, D), norms=True)
    e1, e2 = float(np.abs(V1.reshape(F.shape) - F).max()), float(np.abs(V2.reshape(T.shape) - T).max())
    print(f"pauli strings vs local_paulis: max |dF| = {e1:.3e}; vs local_pair_paulis(max_dist={D}): max |dT| = {e2:.3e}")
    assert e1 < 1e-12 and e2 < 1e-12
    assert np.array_equal(nrm1, nrm) and np.array_equal(nrm2, nrm)


# ---- 4. device-built set and exact state vectors ------------------------------------------------------------------------
def _exact_values(ans, x, S):
    circ = ans.circuit_for_data(x)
    psi = R.statevector(circ.n_qubits, [(name, tuple(qs), (p[0] if p else None)) for name, qs, p in circ.as_tuples()])
    return pauli_strings_from_dense(psi, circ.n_qubits, S)[0]


def test_device_built_set_and_exact_state_vectors(gpu_ctx):
    n = 12
    ans = Q.KernelStateAnsatz(n, 2, 1.0, Q.entanglement_graph(n, 2))
    X = R.synthetic_features(6, n, 21)
    S = case_strings(n, np.random.default_rng(5))
    circs = [ans.circuit_for_data(x) for x in X]
    dset, _, _ = gpu_ctx.build_share(circs, 1 - 1e-16, max_bond=256)
    assert dset is not None
    with dset:
        Vd = gpu_ctx.pauli_expectations(dset, S)
    Vh, _ = _device_values(gpu_ctx, [Q.simulate(c, 1 - 1e-16) for c in circs], S)
    assert np.abs(Vd - Vh).max() < 1e-10
    exact = np.stack([_exact_values(ans, x, S) for x in X])
    share = float((np.abs(exact) >= 1e-3).mean())
    worst = float(np.abs(Vd - exact).max())
    print(f"device-built set vs exact state vectors: max |dV| = {worst:.3e}, share of |exact| >= 1e-3: {share:.2f}")
    assert share >= 0.5 and worst < 1e-10
    # every gate of the ansatz without its Hadamards conserves parity
    ans0 = Q.KernelStateAnsatz(n, 2, 1.0, Q.entanglement_graph(n, 2), hadamard_init=False)
    states = [Q.simulate(ans0.circuit_for_data(x), 1 - 1e-16) for x in X]
    assert max(m.max_bond() for m in states) >= 8
    par = gpu_ctx_values_of(gpu_ctx, states, ["Z" * n])
    assert np.abs(par - 1.0).max() < 1e-10


# ---- 5. bit guarantees --------------------------------------------------------------------------------------------------
def test_bit_guarantees(gpu_ctx, monkeypatch):
    rng = np.random.default_rng(2)
    prof = [1, 2, 4, 8, 16, 32, 64, 100, 64, 32, 16, 8, 4, 2, 1]
    n = 14
    big = [Q.random_mps(n, prof if k % 3 else [min(c, 20) for c in prof], rng) for k in range(40)]
    S = case_strings(n, rng, count=40)
    assert len(S) == 50
    monkeypatch.delenv("QK_STRINGS_BATCH", raising=False)
    alone, _ = _device_values(gpu_ctx, [big[17]], S)
    with gpu_ctx.upload(big) as s:
        V1 = gpu_ctx.pauli_expectations(s, S)
        V2 = gpu_ctx.pauli_expectations(s, S)
        Vr = gpu_ctx.pauli_expectations(s, S[::-1])
        one = gpu_ctx.pauli_expectations(s, S[23:24])
        # 40 x 49 chains (the all-identity string has none): at most 700, then at most 37 chains per batch
        batched = []
        for cap in ("700", "37"):
            monkeypatch.setenv("QK_STRINGS_BATCH", cap)
            batched.append(gpu_ctx.pauli_expectations(s, S))
        monkeypatch.setenv("QK_STRINGS_BATCH", "0")  # read per call: a bad value is an error of that call
        with pytest.raises(engine.QkError, match="QK_STRINGS_BATCH"):
            gpu_ctx.pauli_expectations(s, S)
        monkeypatch.delenv("QK_STRINGS_BATCH")
        V3 = gpu_ctx.pauli_expectations(s, S)
    assert np.array_equal(alone[0], V1[17])
    assert np.array_equal(V1, V2) and np.array_equal(V1, V3)
    assert np.array_equal(Vr, V1[:, ::-1])
    assert np.array_equal(one[:, 0], V1[:, 23])
    for Vb in batched:
        assert np.array_equal(Vb, V1)
    assert np.all(np.abs(V1) <= 1.0 + 1e-12)


# ---- 6. rejections ------------------------------------------------------------------------------------------------------
def test_rejections(gpu_ctx):
    rng = np.random.default_rng(0)
    L = engine.lib()
    out, S = np.zeros((1, 2)), np.array([[0, 3, 1, 0], [2, 0, 0, 0]], dtype=np.uint8)
    with gpu_ctx.upload([Q.random_mps(4, [1, 2, 4, 2, 1], rng)]) as s, s.to_f32() as s32:
        with pytest.raises(engine.QkError, match="complex64"):
            gpu_ctx.pauli_expectations(s32, S)
        bad = S.copy()
        bad[1, 2] = 4
        with pytest.raises(engine.QkError, match=r"strings\[1\]\[2\]"):
            engine._check(L.qk_pauli_strings_host(gpu_ctx._h, s.handle, 2, bad.ctypes.data, out.ctypes.data, None), "strings")
        with pytest.raises(engine.QkError, match="n_strings"):
            engine._check(L.qk_pauli_strings_host(gpu_ctx._h, s.handle, 0, S.ctypes.data, out.ctypes.data, None), "strings")
        for args, name in (((None, s.handle, 2, S.ctypes.data, out.ctypes.data, None), "ctx"), ((gpu_ctx._h, None, 2, S.ctypes.data, out.ctypes.data, None), "set"),
                           ((gpu_ctx._h, s.handle, 2, None, out.ctypes.data, None), "strings"), ((gpu_ctx._h, s.handle, 2, S.ctypes.data, None, None), "out")):
            with pytest.raises(engine.QkError, match=f"{name} is null"):
                engine._check(L.qk_pauli_strings_host(*args), "strings")
        with pytest.raises(ValueError, match="ZXZ"):
            gpu_ctx.pauli_expectations(s, ["IZXI", "ZXZ"])
        with engine.Context(0) as other:
            with pytest.raises(engine.QkError, match="another context"):
                engine._check(L.qk_pauli_strings_host(other._h, s.handle, 2, S.ctypes.data, out.ctypes.data, None), "strings")
        engine._check(L.qk_pauli_strings_host(gpu_ctx._h, s.handle, 2, S.ctypes.data, out.ctypes.data, None), "strings")  # norms may be NULL
    f, k = np.zeros((2, 5)), np.zeros((2, 2))
    for args, match in (((5, 2, f.ctypes.data, 2, None, 0.0, k.ctypes.data, 2), "g must be"), ((5, 2, f.ctypes.data, 2, None, 0.5, k.ctypes.data, 1), "ld"),
                        ((0, 2, f.ctypes.data, 2, None, 0.5, k.ctypes.data, 2), "n_features"), ((5, 2, f.ctypes.data, 3, None, 0.5, k.ctypes.data, 2), "ny 3 != nx 2"),
                        ((5, 2, None, 2, None, 0.5, k.ctypes.data, 2), "null")):
        with pytest.raises(engine.QkError, match=match):
            engine._check(L.qk_feature_gram_host(gpu_ctx._h, *args), "gram")
    with pytest.raises(ValueError, match="bandwidth"):
        gpu_ctx.feature_gram(f, gamma=0.0)


# ---- 7. the feature Gram ------------------------------------------------------------------------------------------------
def ref_feature_gram(fx, fy, g):
    d = fx[None, :, :] - fy[:, None, :]
    return np.exp(-g * (d * d).sum(axis=2))


def test_feature_gram_kernel(gpu_ctx):
    rng = np.random.default_rng(5)
    n = 10
    states = [Q.random_mps(n, [1, 2, 4, 8, 16, 16, 8, 4, 2, 1, 1], rng) for _ in range(70)]
    S = np.vstack([case_strings(n, rng, count=30), weight_one_strings(n)])
    with gpu_ctx.upload(states) as s:
        V = gpu_ctx.pauli_expectations(s, S)
        F = gpu_ctx.local_paulis(s)
    m = V.shape[1]
    K = gpu_ctx.feature_gram(V)
    assert K.shape == (70, 70)
    assert np.abs(K - ref_feature_gram(V, V, 1.0 / m)).max() < 1e-13  # the default bandwidth 1 / n_features
    assert np.array_equal(K, K.T) and np.all(np.diag(K) == 1.0)
    Kr = gpu_ctx.feature_gram(V, V[:23], gamma=0.37)
    assert Kr.shape == (23, 70)
    assert np.abs(Kr - ref_feature_gram(V, V[:23], 0.37)).max() < 1e-13
    # the 3 n weight-1 columns at g / 2 are the one-qubit projected kernel at g
    W = np.ascontiguousarray(V[:, -3 * n:])
    assert np.abs(gpu_ctx.feature_gram(W, gamma=0.37 / 2) - gpu_ctx.projected_gram(F, gamma=0.37)).max() < 1e-13
    assert np.abs(gpu_ctx.feature_gram(W, W[:23], gamma=0.37 / 2) - gpu_ctx.projected_gram(F, F[:23], gamma=0.37)).max() < 1e-13


# ---- 8. build_projected_kernel_matrix(observables=...) ------------------------------------------------------------------
def _observables(n):
    return [row for row in sparse_strings(n, 30, np.random.default_rng(17))] + ["Z" * n, ("XX", (0, n - 1)), ("ZXZ", (3, 4, 5))]


def _exact_kernel(ans, X, Y, g, S):
    fx = np.stack([_exact_values(ans, x, S) for x in X])
    fy = fx if Y is None else np.stack([_exact_values(ans, y, S) for y in Y])
    return ref_feature_gram(fx, fy, g)


@pytest.mark.parametrize("builder", ["device", "host"])
def test_build_projected_kernel_matrix_observables_exact(gpu_ctx, monkeypatch, tmp_path, builder):
    import json

    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_projected_kernel_matrix

    monkeypatch.setenv("QK_BUILDER", builder)
    n = 12
    ans = Q.KernelStateAnsatz(n, 2, 1.0, Q.entanglement_graph(n, 2))
    X, Y = R.synthetic_features(7, n, 8), R.synthetic_features(4, n, 9)
    obs = _observables(n)
    S = engine.pauli_strings(n, obs)
    info = str(tmp_path / "prof")
    K = build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, info_file=info, observables=obs)
    err = float(np.abs(K - _exact_kernel(ans, X, None, 1.0 / len(obs), S)).max())
    print(f"build_projected_kernel_matrix(observables: {len(obs)} strings), {builder} builder: max |dK| = {err:.3e}")
    assert K.shape == (7, 7) and err < 1e-10
    prof = json.load(open(info + ".json"))
    assert prof["pqk_observables"] == [len(obs), "strings"] and "pqk_rdm" not in prof and "pqk_pair_distance" not in prof
    assert prof["pqk_gamma"][0] == 1.0 / len(obs) and "pqk_features_time" in prof and "kernel_mat_time" in prof
    Kt = build_projected_kernel_matrix(SingleComm(), ans, X, Y=Y, pqk_gamma=0.2, truncation_error=1e-16, observables=obs)
    assert Kt.shape == (4, 7) and np.abs(Kt - _exact_kernel(ans, X, Y, 0.2, S)).max() < 1e-10
    # the weight-1 strings at g / 2 are the one-qubit form at g
    K1 = build_projected_kernel_matrix(SingleComm(), ans, X, pqk_gamma=0.3, truncation_error=1e-16, info_file=info, rdm=1)
    assert json.load(open(info + ".json"))["pqk_rdm"] == [1, "qubits"]
    Kw = build_projected_kernel_matrix(SingleComm(), ans, X, pqk_gamma=0.15, truncation_error=1e-16, observables=weight_one_strings(n))
    assert np.abs(Kw - K1).max() < 1e-12


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
        from test_gpu_pauli_strings import _observables as obs_

        n = 10
        ans = Q_.KernelStateAnsatz(n, 2, 1.0, Q_.entanglement_graph(n, 2))
        X, Y = R_.synthetic_features(9, n, 13), R_.synthetic_features(5, n, 14)
        comm = TorchComm()
        out = {"train": build_projected_kernel_matrix(comm, ans, X, truncation_error=1e-16, observables=obs_(n)),
               "test": build_projected_kernel_matrix(comm, ans, X, Y=Y, truncation_error=1e-16, observables=obs_(n))}
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
    port = 29600 + ((os.getpid() + 977) % 2000)
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
    one = build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, observables=_observables(n))
    one_t = build_projected_kernel_matrix(SingleComm(), ans, X, Y=Y, truncation_error=1e-16, observables=_observables(n))
    assert np.array_equal(res[0]["train"], one)
    assert np.array_equal(res[0]["test"], one_t)
