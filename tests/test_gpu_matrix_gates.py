"""GPU tests of the matrix gates (op codes 8 and 9) in the device builder: a Haar brickwork against the host builder and against dense
state vectors, shared and per-state matrix tables, GHZ by a CX chain, snapshots and resume, a capped build, and the rejections of
``qk_build_mps_gates``.

Tolerances as tests/test_gpu_feature_map.py: fidelity within 1e-12 of 1, |<dev|host>|^2 = 1 within 1e-10, Gram entries of the two
state sets within 1e-9, Grams against the exact state vectors within 1e-10; the capped build as
tests/test_gpu_builder.py::test_bond_cap_on_the_block_path: |f_dev - f_host| < 1e-9 max(1, f_host)."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import restatement as R
from test_matrix_gates_host import N_BAD, MatrixGateList, bad_programs, brickwork, dense_state, features, from_gates, mps_vector

pytestmark = pytest.mark.gpu

EXTRAS = [("CX", [7, 6], []), ("CZ", [2, 5], [])]


def circuits_12(npts=3):
    """n = 12, six brickwork layers of Haar Unitary2q with Rz / Ry data layers between them, a CX on [7, 6] and a CZ on [2, 5]: dense
    numpy says the bonds are 2, 4, 8, 16, 32, 64, 32, ... -- the theta product on the matrix cores (bond >= 32) and the preconditioned
    block factorisation (>= 48 columns) both run."""
    n = 12
    return [from_gates(n, brickwork(n, 6, x, seed=17, extras=EXTRAS)) for x in features(npts, n, 41)]


@pytest.fixture(scope="module")
def host_12(built):
    import qml_cutensornet_amd as Q

    circuits = circuits_12()
    return circuits, [Q.simulate(c, 1 - 1e-16) for c in circuits]


@pytest.mark.parametrize("wgs", ["1", "2"])
def test_device_builder_matches_host_builder_on_a_haar_brickwork(gpu_ctx, host_12, monkeypatch, wgs):
    monkeypatch.setenv("QK_BUILD_WGS", wgs)
    circuits, host = host_12
    assert 9 in circuits[0].op and 3 in circuits[0].op  # 4x4 matrix gates, and the SWAP chain of the CZ on [2, 5]
    dev, info = gpu_ctx.build_mps(circuits)
    print(f"matrix gates, n = 12, six Haar layers, 3 states, QK_BUILD_WGS={wgs}: kernel_ms = {info['kernel_ms']:.3f}")
    assert info["kernel_ms"] > 0 and len(dev) == 3
    assert max(m.max_bond() for m in host) == 64 and max(m.max_bond() for m in dev) == 64
    for md, mh in zip(dev, host):
        assert md.max_bond() == 64 and mh.max_bond() == 64
        assert np.array_equal(md.bond_dims(), mh.bond_dims())
        assert abs(md.fidelity - 1.0) < 1e-12
    z = np.array([R.mps_inner(md.tensors, mh.tensors) for md, mh in zip(dev, host)])
    assert np.abs(np.abs(z) ** 2 - 1).max() < 1e-10
    with gpu_ctx.upload(dev) as dx, gpu_ctx.upload(host) as hx:
        assert np.abs(gpu_ctx.gram(dx) - gpu_ctx.gram(hx)).max() < 1e-9


@pytest.mark.parametrize("builder", ["device", "host"])
def test_build_kernel_matrix_with_per_state_tables(built, monkeypatch, builder):
    """The same circuit at n = 10 with every Haar unitary multiplied by a data-dependent diagonal and a data-dependent Unitary1q layer
    (a gate-list ansatz: one matrix table per state), against the dense vectors."""
    from qml_cutensornet_amd.ansatz import as_bound_circuit
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_kernel_matrix

    monkeypatch.setenv("QK_BUILDER", builder)
    n = 10
    gl = MatrixGateList(n, 6, seed=17, extras=EXTRAS)
    X, Y = features(5, n, 51), features(3, n, 52)
    a, b = (as_bound_circuit(gl.circuit_for_data(x), gl) for x in X[:2])
    assert np.array_equal(a.mat, b.mat) and not np.array_equal(a.mats, b.mats)
    sx = [dense_state(n, gl.circuit_for_data(x)) for x in X]
    sy = [dense_state(n, gl.circuit_for_data(y)) for y in Y]
    K = build_kernel_matrix(SingleComm(), gl, X=X, truncation_error=1e-16)
    assert K.shape == (5, 5) and np.abs(K - np.array([[abs(np.vdot(p, q)) ** 2 for p in sx] for q in sx])).max() < 1e-10
    Kt = build_kernel_matrix(SingleComm(), gl, X=X, Y=Y, truncation_error=1e-16)
    assert Kt.shape == (3, 5) and np.abs(Kt - np.array([[abs(np.vdot(p, q)) ** 2 for p in sx] for q in sy])).max() < 1e-10


@pytest.mark.parametrize("builder", ["auto", "hybrid"])
def test_builder_policies_take_a_matrix_table(built, monkeypatch, builder):
    """QK_BUILDER=auto and hybrid with per-state tables: the policies read the cost proxy (which counts the 4x4 gates) and whichever
    builder they choose, the Gram is the dense one.  30 states: the hybrid policy runs its pilot and both builders."""
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_kernel_matrix

    monkeypatch.setenv("QK_BUILDER", builder)
    monkeypatch.setenv("QK_BUILD_WORKERS", "2")
    n = 8
    gl = MatrixGateList(n, 4, seed=23, extras=[("CX", [5, 2], [])])
    X = features(30, n, 61)
    sx = [dense_state(n, gl.circuit_for_data(x)) for x in X]
    K = build_kernel_matrix(SingleComm(), gl, X=X, truncation_error=1e-16)
    assert K.shape == (30, 30) and np.abs(K - np.array([[abs(np.vdot(p, q)) ** 2 for p in sx] for q in sx])).max() < 1e-10


@pytest.mark.parametrize("far", [False, True])
def test_ghz_by_a_cx_chain_on_the_device(gpu_ctx, far):
    n = 8
    if far:  # a non-adjacent CX: qubit 5 is entangled from qubit 0 through a SWAP chain
        gates = [("H", [0], [])] + [("CX", [q, q + 1], []) for q in range(4)] + [("CX", [0, 5], []), ("CX", [5, 6], []), ("CX", [6, 7], [])]
    else:
        gates = [("H", [0], [])] + [("CX", [q, q + 1], []) for q in range(n - 1)]
    dev, _ = gpu_ctx.build_mps([from_gates(n, gates)])
    ghz = np.zeros(2 ** n, dtype=complex)
    ghz[0] = ghz[-1] = 1 / math.sqrt(2.0)
    assert dev[0].bond_dims().tolist() == [1] + [2] * (n - 1) + [1]
    assert abs(abs(np.vdot(ghz, mps_vector(dev[0]))) ** 2 - 1) < 1e-12
    assert abs(dev[0].fidelity - 1) < 1e-12


def _download(h, ns, n):
    from qml_cutensornet_amd.engine import _check, lib

    try:
        dims = np.zeros((ns, n + 1), dtype=np.int32)
        offs = np.zeros(ns, dtype=np.int64)
        total = C.c_int64()
        _check(lib().qk_built_info(h, dims.ctypes.data, None, offs.ctypes.data, C.byref(total), None), "qk_built_info")
        flat = np.empty(total.value, dtype=np.complex128)
        _check(lib().qk_built_download(h, flat.ctypes.data), "qk_built_download")
    finally:
        lib().qk_built_destroy(h)
    sizes = (2 * dims[:, :-1].astype(np.int64) * dims[:, 1:]).sum(axis=1)
    return dims, [flat[o : o + s].copy() for o, s in zip(offs, sizes)]


def test_shared_and_per_state_tables_agree_bit_for_bit(gpu_ctx, host_12):
    """One program with one shared table (stride 0), and again with the same table repeated per state (stride n_mats)."""
    from qml_cutensornet_amd.engine import _GateProgram

    circuits, _ = host_12
    shared = _GateProgram("test", circuits)
    assert shared.stride == 0 and shared.n_mats > 30 and shared.mats.shape == (shared.n_mats, 4, 4)
    dims_a, a = _download(shared.build(gpu_ctx, 1 - 1e-16, 1e-16, 256, 0), 3, 12)
    per_state = _GateProgram("test", circuits)
    per_state.mats, per_state.stride = np.ascontiguousarray(np.stack([shared.mats] * 3)), shared.n_mats
    dims_b, b = _download(per_state.build(gpu_ctx, 1 - 1e-16, 1e-16, 256, 0), 3, 12)
    assert np.array_equal(dims_a, dims_b) and dims_a.max() == 64
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_scan_and_resume_inside_the_brickwork(gpu_ctx, host_12):
    circuits, _ = host_12
    c0 = circuits[0]
    two_q = np.flatnonzero(c0.op == 9)
    cps = [int(two_q[8]) + 1, int(two_q[19]) + 3, int(two_q[27]), c0.n_gates]  # inside layers 2, 4 and 5; the last: the whole program
    with gpu_ctx.build_mps_scan(circuits, cps) as scan:
        assert scan.checkpoints == cps
        final = scan.states(-1)
        whole, _ = gpu_ctx.build_mps(circuits)
        for a, b in zip(final, whole):  # the snapshots are copies: the run is the run without them
            assert all(np.array_equal(x, y) for x, y in zip(a.tensors, b.tensors))
        for j, cp in enumerate(cps[:-1]):
            snap = scan.states(j)
            fresh, _ = gpu_ctx.build_mps([c.sliced(0, cp) for c in circuits])
            for a, b in zip(snap, fresh):
                assert abs(a.fidelity - 1) < 1e-12 and abs(b.fidelity - 1) < 1e-12
                assert abs(abs(R.mps_inner(a.tensors, b.tensors)) ** 2 - 1) < 1e-10
            with scan.set(j) as sx, gpu_ctx.upload(fresh) as fx:
                assert np.abs(gpu_ctx.gram(sx) - gpu_ctx.gram(fx)).max() < 1e-9
            with gpu_ctx.build_mps_scan([c.sliced(cp, c.n_gates) for c in circuits], [c0.n_gates - cp], initial=(scan, j)) as resumed:
                for a, b in zip(resumed.states(-1), final):  # the existing resume guarantee: the bits of the uninterrupted run
                    assert a.fidelity == b.fidelity and all(np.array_equal(x, y) for x, y in zip(a.tensors, b.tensors))


def test_capped_device_build(gpu_ctx, host_12):
    import qml_cutensornet_amd as Q

    circuits, _ = host_12
    host = [Q.simulate(c, 1 - 1e-16, max_bond=8) for c in circuits]
    dev, info = gpu_ctx.build_mps(circuits, max_bond=8, truncate=True)
    assert not info["dropped"]
    for d, h in zip(dev, host):
        print(f"capped at 8: device fidelity {d.fidelity:.15e}, host {h.fidelity:.15e}, difference {d.fidelity - h.fidelity:.3e}")
        assert d.max_bond() <= 8 and d.bond_dims().max() == 8 and d.fidelity < 1 - 1e-3
        assert abs(d.fidelity - h.fidelity) < 1e-9 * max(1.0, h.fidelity)


@pytest.mark.parametrize("case", range(1, N_BAD + 1))
def test_device_entry_rejects_bad_matrix_gates(gpu_ctx, case):
    """The list of tests/test_matrix_gates_host.py through ``qk_build_mps_gates``: each a QkError raised by the checks in front of the
    launch (the message names the gate's position, which the kernel's error bits cannot)."""
    from qml_cutensornet_amd.engine import QkError

    _, ok, _ = bad_programs()[0]
    dev, _ = gpu_ctx.build_mps([ok, ok])
    assert abs(dev[0].fidelity - 1) < 1e-12
    label, c, text = bad_programs()[case]
    in_table = label in ("not unitary", "not unitary by 2e-9", "NaN")  # op, q0 and mat of the good program: the bad table is state 1's
    with pytest.raises(QkError, match="gate 2 on a qubit" if text == "outside" else (text if not text.startswith("gate") else "gate [12]: ")):
        gpu_ctx.build_mps([ok, c] if in_table else [c, c])
