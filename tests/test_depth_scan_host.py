"""CPU tests of the depth scan: the prefix property of the layered ansatz that makes a scan possible, ``BoundCircuit.sliced``, the
host mirror ``simulate(..., checkpoints=)`` against plain builds of the shallower circuits and against exact state vectors, and the
argument checks of every layer.

Tolerances: a snapshot and the plain build of the shallower circuit do the same arithmetic up to and including the last truncation
and differ only in where the singular values go after the last two-qubit gate, so bond tables and fidelities are EQUAL and the
normalised overlap is within 1e-10 of 1 (the builder-against-builder bound of tests/test_gpu_builder.py); against exact state
vectors 1e-8, the bound every builder is held to."""
import numpy as np
import pytest

CASES = [(8, 3, 1), (12, 3, 2), (14, 4, 2)]  # qubits, layers, entanglement distance


def _overlap_defect(a, b):
    from oracle import restatement as R

    z = R.mps_inner(a.tensors, b.tensors)
    return abs(abs(z) ** 2 / (R.mps_inner(a.tensors, a.tensors).real * R.mps_inner(b.tensors, b.tensors).real) - 1.0)


@pytest.fixture
def numpy_builder(monkeypatch):
    monkeypatch.setenv("QK_NATIVE_BUILDER", "0")


@pytest.mark.parametrize("n,reps,d", CASES)
def test_shallower_ansatz_is_a_prefix_of_the_deeper_one(n, reps, d):
    import qml_cutensornet_amd as Q
    from oracle import restatement as R

    x = R.synthetic_features(3, n, 7)[1]
    edges = Q.entanglement_graph(n, d)
    deep = Q.KernelStateAnsatz(n, reps, 1.0, edges)
    ends = deep.layer_ends()
    c = deep.circuit_for_data(x)
    assert len(ends) == reps and ends[-1] == c.n_gates and all(b > a for a, b in zip(ends, ends[1:]))
    assert ends[0] - n == ends[1] - ends[0]  # n Hadamards, then equal layers
    for r in range(1, reps + 1):
        s = Q.KernelStateAnsatz(n, r, 1.0, edges).circuit_for_data(x)
        e = ends[r - 1]
        assert s.n_gates == e
        assert np.array_equal(s.op, c.op[:e]) and np.array_equal(s.q0, c.q0[:e]) and np.array_equal(s.alpha, c.alpha[:e])
        p = c.sliced(0, e)
        assert p.n_qubits == n and np.array_equal(p.op, s.op) and np.array_equal(p.q0, s.q0) and np.array_equal(p.alpha, s.alpha)
    assert Q.KernelStateAnsatz(n, reps, 1.0, edges, hadamard_init=False).layer_ends()[0] == ends[0] - n


@pytest.mark.parametrize("n,reps,d", CASES)
def test_sliced_composes(n, reps, d):
    import qml_cutensornet_amd as Q
    from oracle import restatement as R

    c = Q.KernelStateAnsatz(n, reps, 1.0, Q.entanglement_graph(n, d)).circuit_for_data(R.synthetic_features(2, n, 7)[0])
    for cut in (0, 1, n + 3, c.n_gates // 2, c.n_gates):
        a, b = c.sliced(0, cut), c.sliced(cut, c.n_gates)
        assert a.n_qubits == b.n_qubits == n and a.n_gates == cut and b.n_gates == c.n_gates - cut
        assert np.array_equal(np.concatenate([a.op, b.op]), c.op)
        assert np.array_equal(np.concatenate([a.q0, b.q0]), c.q0)
        assert np.array_equal(np.concatenate([a.alpha, b.alpha]), c.alpha)
        assert a.op.dtype == c.op.dtype and a.q0.dtype == c.q0.dtype
    inner = c.sliced(5, 40).sliced(3, 10)
    assert np.array_equal(inner.op, c.op[8:15]) and np.array_equal(inner.alpha, c.alpha[8:15])
    for bad in ((-1, 3), (4, 3), (0, c.n_gates + 1)):
        with pytest.raises(ValueError):
            c.sliced(*bad)


def test_custom_feature_map_takes_arbitrary_checkpoints(numpy_builder):
    import qml_cutensornet_amd as Q

    n = 6
    gates = [("H", [q], None) for q in range(n)]
    for _ in range(2):
        gates += [("Ry", [q], (0.5, (q, 0.0, 1.0))) for q in range(n)]
        gates += [("ZZPhase", [a, b], (0.7, (a, 1.0, -1.0), (b, 1.0, -1.0))) for a, b in ((0, 1), (2, 4), (3, 5), (1, 2))]
    ans = Q.CircuitAnsatz(n, gates)
    c = ans.circuit_for_data(np.linspace(0.1, 1.9, n))
    assert ans.layer_ends() == [c.n_gates]
    cps = [3, n + 7, c.n_gates - 2, c.n_gates]
    snaps = Q.simulate(c, checkpoints=cps)
    assert len(snaps) == len(cps)
    for m, e in zip(snaps, cps):
        plain = Q.simulate(c.sliced(0, e))
        assert np.array_equal(m.bond_dims(), plain.bond_dims()) and m.fidelity == plain.fidelity
        assert _overlap_defect(m, plain) < 1e-10


@pytest.mark.parametrize("n,reps,d", CASES)
def test_host_mirror_last_snapshot_is_the_plain_build_bit_for_bit(numpy_builder, n, reps, d):
    import qml_cutensornet_amd as Q
    from oracle import restatement as R

    ans = Q.KernelStateAnsatz(n, reps, 1.0, Q.entanglement_graph(n, d))
    for x in R.synthetic_features(2, n, 7):
        c = ans.circuit_for_data(x)
        snaps = Q.simulate(c, checkpoints=ans.layer_ends())
        plain = Q.simulate(c)
        assert isinstance(snaps, list) and len(snaps) == reps
        assert snaps[-1].fidelity == plain.fidelity
        assert all(np.array_equal(a, b) for a, b in zip(snaps[-1].tensors, plain.tensors))
        one = Q.simulate(c, checkpoints=[c.n_gates])
        assert len(one) == 1 and all(np.array_equal(a, b) for a, b in zip(one[0].tensors, plain.tensors))


def test_host_mirror_runs_the_numpy_loop_whatever_the_native_switch_says(monkeypatch):
    import qml_cutensornet_amd as Q
    from oracle import restatement as R

    ans = Q.KernelStateAnsatz(8, 2, 1.0, Q.entanglement_graph(8, 1))
    c = ans.circuit_for_data(R.synthetic_features(2, 8, 7)[0])
    monkeypatch.setenv("QK_NATIVE_BUILDER", "1")
    a = Q.simulate(c, checkpoints=ans.layer_ends())
    monkeypatch.setenv("QK_NATIVE_BUILDER", "0")
    b = Q.simulate(c, checkpoints=ans.layer_ends())
    for ma, mb in zip(a, b):
        assert ma.fidelity == mb.fidelity and all(np.array_equal(s, t) for s, t in zip(ma.tensors, mb.tensors))


@pytest.mark.parametrize("n,reps,d", CASES)
def test_host_mirror_earlier_snapshots_against_plain_builds(numpy_builder, n, reps, d):
    import qml_cutensornet_amd as Q
    from oracle import restatement as R

    edges = Q.entanglement_graph(n, d)
    deep = Q.KernelStateAnsatz(n, reps, 1.0, edges)
    for x in R.synthetic_features(2, n, 7):
        snaps = Q.simulate(deep.circuit_for_data(x), checkpoints=deep.layer_ends())
        for r in range(1, reps + 1):
            plain = Q.simulate(Q.KernelStateAnsatz(n, r, 1.0, edges).circuit_for_data(x))
            assert np.array_equal(snaps[r - 1].bond_dims(), plain.bond_dims())
            assert snaps[r - 1].fidelity == plain.fidelity
            assert _overlap_defect(snaps[r - 1], plain) < 1e-10


def test_host_mirror_truncating_run_keeps_the_fidelity_so_far(numpy_builder):
    """A loose budget really truncates: a snapshot's fidelity is the product up to its gate, not the final one."""
    import qml_cutensornet_amd as Q
    from oracle import restatement as R

    n, reps = 14, 3
    edges = Q.entanglement_graph(n, 2)
    deep = Q.KernelStateAnsatz(n, reps, 1.0, edges)
    x = R.synthetic_features(4, n, 11)[0]
    snaps = Q.simulate(deep.circuit_for_data(x), 1 - 1e-4, checkpoints=deep.layer_ends())
    fids = [m.fidelity for m in snaps]
    assert fids[0] < 1.0 and all(b < a for a, b in zip(fids, fids[1:]))
    for r in range(1, reps + 1):
        plain = Q.simulate(Q.KernelStateAnsatz(n, r, 1.0, edges).circuit_for_data(x), 1 - 1e-4)
        assert snaps[r - 1].fidelity == plain.fidelity and np.array_equal(snaps[r - 1].bond_dims(), plain.bond_dims())


def test_host_mirror_against_exact_statevectors(numpy_builder):
    import qml_cutensornet_amd as Q
    from oracle import restatement as R

    n, reps = 8, 3
    edges = Q.entanglement_graph(n, 1)
    X = R.synthetic_features(6, n, 7)
    deep = Q.KernelStateAnsatz(n, reps, 1.0, edges)
    snaps = [Q.simulate(deep.circuit_for_data(x), checkpoints=deep.layer_ends()) for x in X]
    exact = [R.gram_statevector(X, None, r, 1.0, edges) for r in range(1, reps + 1)]
    for r in range(1, reps + 1):
        K = R.gram_from_mps([s[r - 1].tensors for s in snaps])
        assert np.abs(K - exact[r - 1]).max() < 1e-8
    # the depths are told apart: a snapshot of the wrong depth would miss by far more than the tolerance
    assert np.abs(exact[0] - exact[1]).max() > 0.05 and np.abs(exact[1] - exact[2]).max() > 0.05


BAD_CHECKPOINTS = {  # N = gates of the program
    "empty": lambda N: [],
    "repeated": lambda N: [5, 5, N],
    "decreasing": lambda N: [7, 3, N],
    "zero": lambda N: [0, N],
    "negative": lambda N: [-2, N],
    "beyond the program": lambda N: [3, N + 1],
    "not ending at the program": lambda N: [3, 12],
    "fractional": lambda N: [2.5, N],
    "not a list of numbers": lambda N: "ab",
}


@pytest.mark.parametrize("case", sorted(BAD_CHECKPOINTS))
def test_checkpoint_errors(case, numpy_builder):
    import qml_cutensornet_amd as Q
    from qml_cutensornet_amd import engine
    from qml_cutensornet_amd.ansatz import check_checkpoints
    from oracle import restatement as R

    c = Q.KernelStateAnsatz(6, 2, 1.0, Q.entanglement_graph(6, 1)).circuit_for_data(R.synthetic_features(2, 6, 7)[0])
    bad = BAD_CHECKPOINTS[case](c.n_gates)
    with pytest.raises(ValueError):
        check_checkpoints(bad, c.n_gates)
    with pytest.raises(ValueError):
        Q.simulate(c, checkpoints=bad)
    ctx = engine.Context.__new__(engine.Context)  # the engine validates before it touches the library or a device
    with pytest.raises(ValueError):
        ctx.build_mps_scan([c], bad)
    assert check_checkpoints([3, np.int32(9), c.n_gates], c.n_gates) == [3, 9, c.n_gates]


@pytest.mark.parametrize("bad", [(), (0,), (4,), (1, 1), (2, 3, 2), (1.5,), (True,), 3])
def test_depth_errors(bad):
    import qml_cutensornet_amd as Q
    from qml_cutensornet_amd.ansatz import check_depths
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_depth_scan_kernel_matrices
    from oracle import restatement as R

    ans = Q.KernelStateAnsatz(6, 3, 1.0, Q.entanglement_graph(6, 1))
    X = R.synthetic_features(3, 6, 7)
    with pytest.raises(ValueError):
        check_depths(bad, ans.reps)
    with pytest.raises(ValueError, match="depths"):
        build_depth_scan_kernel_matrices(SingleComm(), ans, X, depths=bad, truncation_error=1e-16)
    assert check_depths((3, 1), 3) == [3, 1]


def test_depth_scan_module_surface_errors():
    import qml_cutensornet_amd as Q
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_depth_scan_kernel_matrices
    from oracle import restatement as R

    ans = Q.KernelStateAnsatz(6, 3, 1.0, Q.entanglement_graph(6, 1))
    X = R.synthetic_features(4, 6, 7)
    with pytest.raises(ValueError, match="truncation error"):
        build_depth_scan_kernel_matrices(SingleComm(), ans, X, depths=(1, 2))
    with pytest.raises(ValueError, match="smaller"):
        build_depth_scan_kernel_matrices(SingleComm(), ans, X[:2], X, depths=(1, 2), truncation_error=1e-16)


def test_new_symbols_are_declared_and_bound(built):
    from qml_cutensornet_amd import engine

    L = engine.lib()
    for name in ("qk_build_mps_scan", "qk_built_num_snapshots", "qk_built_checkpoints", "qk_built_info_at", "qk_built_download_at", "qk_mps_set_from_built_at"):
        assert name in engine.EXPORTED_SYMBOLS and hasattr(L, name)
