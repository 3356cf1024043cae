"""GPU tests of the device builder's snapshots and resume (``Context.build_mps_scan``) and of ``build_depth_scan_kernel_matrices``.

Sets.  A: 14 qubits x 4 layers, distance 2, gamma 1, three points, default budget and ``max_bond`` -- the host builder's largest
bonds are 4 / 16 / 33 / 53 at depths 1..4, so depths 1-2 factorise in LDS and from depth 3 the thetas have >= 48 columns and go
through the preconditioned block Jacobi; the default ``max_bond`` gives the 512-thread shape.  B: 12 qubits x 3 layers, distance 2,
``max_bond=32``: the four-workgroup 256-thread shape.  A again under QK_BUILD_WGS=2 with ``max_bond=64, truncate=True``: the
two-workgroup shape with the cap switched on (it lies above this set's largest bond, 53).

Tolerances.  A snapshot is a copy, so the last snapshot of a scan IS the plain build and a resumed build IS the uninterrupted one:
bit for bit -- provided the builder repeats itself from run to run, which ``reproducible`` checks first on two plain builds of set A
(if it does not, "bit for bit" reads "equal bond tables, equal fidelity, overlap within 1e-10 of 1" everywhere below, and the PR that
finds this says so).  Snapshot r against the plain build of the r-layer circuit: the same arithmetic up to and including the last
truncation, only the placement of the singular values after the last two-qubit gate differs -- equal bond tables, equal fidelity,
normalised overlap within 1e-10 of 1 and Grams within 1e-9 (the builder-against-builder bounds of tests/test_gpu_builder.py).
Against exact state vectors 1e-8 (the bound every builder is held to)."""
import json

import numpy as np
import pytest

from helpers import golden

pytestmark = pytest.mark.gpu


def _overlap_defect(a, b):
    from oracle import restatement as R

    z = R.mps_inner(a.tensors, b.tensors)
    return abs(abs(z) ** 2 / (R.mps_inner(a.tensors, a.tensors).real * R.mps_inner(b.tensors, b.tensors).real) - 1.0)


def _same_bits(a, b):
    return (a.fidelity == b.fidelity and np.array_equal(a.bond_dims(), b.bond_dims())
            and all(np.array_equal(s, t) for s, t in zip(a.tensors, b.tensors)))


def _assert_same(xs, ys, reproducible, what):
    """bit for bit -- or, on a builder that does not repeat itself, equal bonds and fidelity and overlap within 1e-10 of 1"""
    assert len(xs) == len(ys)
    for k, (a, b) in enumerate(zip(xs, ys)):
        assert np.array_equal(a.bond_dims(), b.bond_dims()), f"{what}: state {k}: bond tables differ"
        assert a.fidelity == b.fidelity, f"{what}: state {k}: fidelity {a.fidelity!r} != {b.fidelity!r}"
        if reproducible:
            assert _same_bits(a, b), f"{what}: state {k}: tensors differ"
        else:
            assert _overlap_defect(a, b) < 1e-10, f"{what}: state {k}"


class _Case:
    """the circuits of one set, deep and per depth, and what to build them with"""

    def __init__(self, n, reps, d, X, **kw):
        import qml_cutensornet_amd as Q

        self.n, self.reps, self.X, self.kw = n, reps, X, kw
        self.edges = Q.entanglement_graph(n, d)
        self.deep = Q.KernelStateAnsatz(n, reps, 1.0, self.edges)
        self.ends = self.deep.layer_ends()
        self.circuits = [self.deep.circuit_for_data(x) for x in X]

    def at_depth(self, r):
        import qml_cutensornet_amd as Q

        ans = Q.KernelStateAnsatz(self.n, r, 1.0, self.edges)
        return [ans.circuit_for_data(x) for x in self.X]


@pytest.fixture(scope="module")
def case_a():
    return _Case(14, 4, 2, np.random.default_rng(5).uniform(0, 2, (3, 14)))


@pytest.fixture(scope="module")
def case_b():
    from oracle import restatement as R

    return _Case(12, 3, 2, R.synthetic_features(5, 12, 7), max_bond=32)


@pytest.fixture(scope="module")
def plain_a(gpu_ctx, case_a):
    """two plain builds of set A: (the states, are the two the same bits?)"""
    one, _ = gpu_ctx.build_mps(case_a.circuits)
    two, _ = gpu_ctx.build_mps(case_a.circuits)
    same = all(_same_bits(a, b) for a, b in zip(one, two))
    print(f"two plain builds of set A are {'the same bits' if same else 'NOT the same bits'}")
    return one, same


@pytest.fixture(scope="module")
def reproducible(plain_a):
    return plain_a[1]


@pytest.fixture(scope="module")
def scan_a(gpu_ctx, case_a):
    with gpu_ctx.build_mps_scan(case_a.circuits, case_a.ends) as scan:
        yield scan


@pytest.fixture(scope="module")
def scan_b(gpu_ctx, case_b):
    with gpu_ctx.build_mps_scan(case_b.circuits, case_b.ends, **case_b.kw) as scan:
        yield scan


@pytest.fixture(scope="module")
def host_a(case_a):
    import qml_cutensornet_amd as Q

    return [Q.simulate(c, checkpoints=case_a.ends) for c in case_a.circuits]


@pytest.fixture(scope="module")
def host_b(case_b):
    import qml_cutensornet_amd as Q

    return [Q.simulate(c, checkpoints=case_b.ends) for c in case_b.circuits]


def test_set_a_reaches_the_block_factorisation(scan_a, case_a, plain_a):
    """the premise of set A: bonds beyond 48 from depth 3 on, small ones before; and the two plain builds agree on the bonds"""
    top = [int(scan_a.info(j)["dims"].max()) for j in range(4)]
    print(f"set A: largest bonds {top}; plain builds repeat bit for bit: {plain_a[1]}")
    assert top[0] <= 4 and top[1] <= 16 and top[2] >= 24 and top[3] >= 48
    assert scan_a.checkpoints == case_a.ends and len(scan_a) == 4 and scan_a.kernel_ms > 0
    assert scan_a.launch["threads"] == 512 and scan_a.launch["grid"] == 3 and scan_a.info(0)["threads"] == 512  # the default max_bond: the 512-thread shape


# ---- 1. the last snapshot is the plain build
def test_last_snapshot_is_the_plain_build_a(scan_a, plain_a, reproducible):
    _assert_same(scan_a.states(3), plain_a[0], reproducible, "set A")
    _assert_same(scan_a.states(-1), plain_a[0], reproducible, "set A, index -1")


def test_last_snapshot_is_the_plain_build_b(gpu_ctx, scan_a, scan_b, case_b, reproducible):
    plain, info = gpu_ctx.build_mps(case_b.circuits, **case_b.kw)
    for launch in (scan_b.launch, info):  # max_bond=32: four 256-thread workgroups per CU (set A's shape has one per CU)
        assert launch["threads"] == 256 and launch["slots"] == 4 * scan_a.launch["slots"] and launch["grid"] == 5
    _assert_same(scan_b.states(2), plain, reproducible, "set B")


def test_two_workgroup_shape_with_a_cap_that_bites(gpu_ctx, scan_a, case_a, reproducible, monkeypatch):
    """QK_BUILD_WGS=2, max_bond=64, truncate: the last snapshot is the plain build, the earlier ones the shallower builds"""
    monkeypatch.setenv("QK_BUILD_WGS", "2")
    kw = dict(max_bond=64, truncate=True)
    plain, info = gpu_ctx.build_mps(case_a.circuits, **kw)
    with gpu_ctx.build_mps_scan(case_a.circuits, case_a.ends, **kw) as scan:
        for launch in (scan.launch, info):  # two 256-thread workgroups per CU
            assert launch["threads"] == 256 and launch["slots"] == 2 * scan_a.launch["slots"]
        snaps = [scan.states(j) for j in range(4)]
        grams = []
        for j in range(4):
            with scan.set(j) as xs:
                grams.append(gpu_ctx.gram(xs))
    _assert_same(snaps[3], plain, reproducible, "QK_BUILD_WGS=2")
    assert max(m.max_bond() for m in plain) <= 64
    # (the largest bond of this set is 53 and no theta keeps more than 64 values, so this cap never cuts: the case covers the shape
    # and the truncate flag, and a cap that did cut would cut the scan and the plain build alike)
    print(f"QK_BUILD_WGS=2, cap 64: largest bond {max(m.max_bond() for m in plain)}, lowest fidelity 1 - {1 - min(m.fidelity for m in plain):.2e}")
    for r in range(1, 4):
        shallow, _ = gpu_ctx.build_mps(case_a.at_depth(r), **kw)
        for a, b in zip(snaps[r - 1], shallow):
            assert np.array_equal(a.bond_dims(), b.bond_dims()) and a.fidelity == b.fidelity
            assert _overlap_defect(a, b) < 1e-10
        with gpu_ctx.upload(shallow) as xs:
            assert np.abs(gpu_ctx.gram(xs) - grams[r - 1]).max() < 1e-9


# ---- 2. snapshot r against the plain build of the r-layer circuits
def _check_against_shallow_builds(ctx, scan, case):
    for r in range(1, case.reps + 1):
        plain, _ = ctx.build_mps(case.at_depth(r), **case.kw)
        snap = scan.states(r - 1)
        worst = 0.0
        for a, b in zip(snap, plain):
            assert np.array_equal(a.bond_dims(), b.bond_dims()), f"depth {r}"
            assert a.fidelity == b.fidelity, f"depth {r}: {a.fidelity!r} != {b.fidelity!r}"
            worst = max(worst, _overlap_defect(a, b))
        with scan.set(r - 1) as xs, ctx.upload(plain) as ps:
            dk = float(np.abs(ctx.gram(xs) - ctx.gram(ps)).max())
        print(f"depth {r}: largest bond {max(m.max_bond() for m in snap)}, overlap defect {worst:.2e}, Gram difference {dk:.2e}")
        assert worst < 1e-10 and dk < 1e-9


def test_snapshots_against_shallower_builds_a(gpu_ctx, scan_a, case_a):
    _check_against_shallow_builds(gpu_ctx, scan_a, case_a)


def test_snapshots_against_shallower_builds_b(gpu_ctx, scan_b, case_b):
    _check_against_shallow_builds(gpu_ctx, scan_b, case_b)


# ---- 3. against the host mirror
def _check_against_host(ctx, scan, host, reps):
    for j in range(reps):
        snap, mirror = scan.states(j), [h[j] for h in host]
        worst = max(_overlap_defect(a, b) for a, b in zip(snap, mirror))
        with scan.set(j) as xs, ctx.upload(mirror) as hs:
            dk = float(np.abs(ctx.gram(xs) - ctx.gram(hs)).max())
        print(f"snapshot {j}: overlap defect against the host mirror {worst:.2e}, Gram difference {dk:.2e}")
        assert worst < 1e-10 and dk < 1e-9
        for a, b in zip(snap, mirror):
            assert abs(a.fidelity - b.fidelity) < 1e-12


def test_snapshots_against_the_host_mirror_a(gpu_ctx, scan_a, host_a):
    _check_against_host(gpu_ctx, scan_a, host_a, 4)


def test_snapshots_against_the_host_mirror_b(gpu_ctx, scan_b, host_b):
    _check_against_host(gpu_ctx, scan_b, host_b, 3)


# ---- 4. against exact state vectors
def test_snapshots_against_exact_statevectors(gpu_ctx):
    import qml_cutensornet_amd as Q
    from oracle import restatement as R

    n, reps = 8, 3
    edges = Q.entanglement_graph(n, 1)
    X = R.synthetic_features(6, n, 7)
    deep = Q.KernelStateAnsatz(n, reps, 1.0, edges)
    with gpu_ctx.build_mps_scan([deep.circuit_for_data(x) for x in X], deep.layer_ends()) as scan:
        for r in range(1, reps + 1):
            with scan.set(r - 1) as xs:
                K = gpu_ctx.gram(xs)
            assert np.abs(K - R.gram_statevector(X, None, r, 1.0, edges)).max() < 1e-8, f"depth {r}"


# ---- 5. resume
@pytest.mark.parametrize("start", [0, 2])
def test_resumed_build_is_the_uninterrupted_one(gpu_ctx, scan_a, case_a, reproducible, start):
    ends = case_a.ends
    before = [scan_a.states(j) for j in range(4)]
    rest = [c.sliced(ends[start], ends[3]) for c in case_a.circuits]
    with gpu_ctx.build_mps_scan(rest, [e - ends[start] for e in ends[start + 1:]], initial=(scan_a, start)) as resumed:
        assert len(resumed) == 3 - start
        for k in range(len(resumed)):
            _assert_same(resumed.states(k), before[start + 1 + k], reproducible, f"resumed from {start}, snapshot {k}")
            assert np.array_equal(resumed.info(k)["centre"], scan_a.info(start + 1 + k)["centre"])
    if start == 2:
        assert max(m.max_bond() for m in before[2]) > 24  # a start from bonds beyond the smallest shape's
    for j in range(4):  # the source is left untouched
        assert all(_same_bits(a, b) for a, b in zip(scan_a.states(j), before[j]))


def test_resume_one_depth_at_a_time(gpu_ctx, scan_a, case_a):
    """A scan walked with one depth in the heap at a time reaches the states of the one-launch scan.  Not their bits: each leg is a
    build that ends at its depth, so the look-ahead after its last two-qubit gate sees the end of the program where the one-launch
    scan sees the next layer, and the legs continue from the other gauge -- the same states to the builder-against-builder bound."""
    ends = case_a.ends
    cur = gpu_ctx.build_mps_scan([c.sliced(0, ends[0]) for c in case_a.circuits], [ends[0]])
    try:
        for r in range(1, 4):
            nxt = gpu_ctx.build_mps_scan([c.sliced(ends[r - 1], ends[r]) for c in case_a.circuits], [ends[r] - ends[r - 1]], initial=(cur, 0))
            cur.close()
            cur = nxt
            for a, b in zip(cur.states(0), scan_a.states(r)):
                assert abs(a.fidelity - b.fidelity) < 1e-12 and _overlap_defect(a, b) < 1e-10, f"walk, depth {r + 1}"
    finally:
        cur.close()


# ---- 6. a snapshot is a set like any other
def test_snapshot_sets_feed_the_engine(gpu_ctx, scan_a):
    for j in (0, 3):
        info = scan_a.info(j)
        assert info["centre"].shape == (3,) and ((info["centre"] >= 0) & (info["centre"] < 14)).all()
        assert (info["fidelity"] > 0).all() and info["heap_bytes"] == 16 * int((2 * info["dims"][:, :-1] * info["dims"][:, 1:]).sum())
        with scan_a.set(j) as xs:
            assert np.array_equal(xs.dims, info["dims"]) and len(xs) == 3
            assert np.array_equal(xs.image()[2], info["dims"])
            K = gpu_ctx.gram(xs)
            assert np.abs(np.diag(K) - 1).max() < 1e-9
            F = gpu_ctx.local_paulis(xs)
            with gpu_ctx.upload(scan_a.states(j)) as hs:  # the same tensors through the host: the two packings agree to rounding
                assert np.abs(F - gpu_ctx.local_paulis(hs)).max() < 1e-12
            with gpu_ctx.compress(xs, max_bond=8) as cs:
                assert cs.dims.max() <= 8 and gpu_ctx.gram(cs).shape == (3, 3)
    scan_a.states(0)  # the scan is still alive after its sets are closed


def test_custom_feature_map_with_checkpoints_inside_a_layer(gpu_ctx):
    import qml_cutensornet_amd as Q

    n = 7
    gates = [("H", [q], None) for q in range(n)]
    for _ in range(2):
        gates += [("Ry", [q], (0.5, (q, 0.0, 1.0))) for q in range(n)]
        gates += [("ZZPhase", [a, b], (0.7, (a, 1.0, -1.0), (b, 1.0, -1.0))) for a, b in ((0, 1), (2, 5), (3, 6), (1, 2), (4, 5))]
    ans = Q.CircuitAnsatz(n, gates)
    cs = [ans.circuit_for_data(x) for x in np.random.default_rng(3).uniform(0, 2, (3, n))]
    cps = [5, n + 9, cs[0].n_gates - 3, cs[0].n_gates]
    host = [Q.simulate(c, checkpoints=cps) for c in cs]
    with gpu_ctx.build_mps_scan(cs, cps, max_bond=32) as scan:
        for j in range(len(cps)):
            for a, h in zip(scan.states(j), host):
                assert np.array_equal(a.bond_dims(), h[j].bond_dims()) and _overlap_defect(a, h[j]) < 1e-10


# ---- 7. what the library refuses
def test_scan_rejects_bad_input(gpu_ctx, scan_a, case_a):
    from qml_cutensornet_amd import engine
    from qml_cutensornet_amd.engine import QkError

    ends = case_a.ends
    rest = [c.sliced(ends[0], ends[3]) for c in case_a.circuits]
    tail = [e - ends[0] for e in ends[1:]]
    with pytest.raises(QkError, match="QK_BUILD_PARTIAL"):
        gpu_ctx.build_mps_scan(case_a.circuits, ends[:2] + ends[3:], partial=True)
    with pytest.raises(QkError, match="QK_BUILD_PARTIAL"):
        gpu_ctx.build_mps_scan(rest, tail[-1:], initial=(scan_a, 0), partial=True)
    other = engine.Context(0)
    try:
        with pytest.raises(QkError, match="another context"):
            other.build_mps_scan(rest, tail, initial=(scan_a, 0))
    finally:
        other.close()
    with pytest.raises(QkError, match="states"):
        gpu_ctx.build_mps_scan(rest[:2], tail, initial=(scan_a, 0))
    last = [c.sliced(ends[2], ends[3]) for c in case_a.circuits]
    with pytest.raises(QkError, match="max_bond"):
        gpu_ctx.build_mps_scan(last, [ends[3] - ends[2]], initial=(scan_a, 2), max_bond=16)
    with pytest.raises(IndexError):
        gpu_ctx.build_mps_scan(rest, tail, initial=(scan_a, 4))
    with gpu_ctx.build_mps_scan(case_a.circuits[:1], [ends[3]], partial=True) as one:  # partial with one checkpoint is build_mps
        assert len(one) == 1


# ---- 8. the module surface
def test_build_depth_scan_kernel_matrices(built, tmp_path, monkeypatch):
    import qml_cutensornet_amd as Q
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import KernelStateAnsatz, build_depth_scan_kernel_matrices
    from oracle import restatement as R

    g = golden("deep_10q_r3_d3.npz")
    n, reps, gamma, d = int(g["n"]), int(g["reps"]), float(g["gamma"]), int(g["d"])
    assert reps == 3
    edges = Q.entanglement_graph(n, d)
    ans = KernelStateAnsatz(num_qubits=n, reps=reps, gamma=gamma, entanglement_map=edges, hadamard_init=True)
    info = str(tmp_path / "scan_info")
    out = build_depth_scan_kernel_matrices(SingleComm(), ans, g["X_train"], depths=(1, 3), truncation_error=1e-16, info_file=info)
    assert out["depths"] == [1, 3] and sorted(out["K"]) == [1, 3]
    assert np.abs(out["K"][3] - g["K_train"]).max() < 1e-8
    assert np.abs(out["K"][1] - R.gram_statevector(g["X_train"], None, 1, gamma, edges)).max() < 1e-8
    nx = len(g["X_train"])
    for r in (1, 3):
        assert out["fidelity"][r].shape == (nx,) and np.abs(out["fidelity"][r] - 1).max() < 1e-9
        assert out["bond_dims"][r].shape == (nx, n + 1) and (out["bond_dims"][r][:, [0, -1]] == 1).all()
    assert out["bond_dims"][1].max() < out["bond_dims"][3].max()
    prof = json.load(open(info + ".json"))
    for key in ("depths", "r0_circ_sim", "kernel_mat_time", "max_chi", "total_time", "lenX"):
        assert key in prof
    assert prof["depths"][0] == [1, 3] and len(prof["kernel_mat_time"][0]) == 2
    assert prof["max_chi"][0] == [int(out["bond_dims"][r].max()) for r in (1, 3)]
    xy = build_depth_scan_kernel_matrices(SingleComm(), ans, g["X_train"], g["X_test"], depths=(1, 3), truncation_error=1e-16)
    assert np.abs(xy["K"][3] - g["K_test"]).max() < 1e-8
    assert np.abs(xy["K"][1] - R.gram_statevector(g["X_train"], g["X_test"], 1, gamma, edges)).max() < 1e-8
    assert xy["fidelity"][3].shape == (nx + len(g["X_test"]),)
