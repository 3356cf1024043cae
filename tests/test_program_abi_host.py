"""CPU tier: the structs of the gate program (``include/qkgram.h``: ``qk_program``, ``qk_build_run``; ``csrc/qk_builder.h``: ``qkb_run``,
``qkb_result``) as ``qml_cutensornet_amd.program`` mirrors them: the sizes agree with both libraries, a struct of another size is
refused by either entry before anything else is looked at, and ``fill_program`` puts every array where its field is."""
import ctypes as C

import numpy as np

from qml_cutensornet_amd import program as P


def test_struct_sizes_agree_with_both_libraries(built):
    from qml_cutensornet_amd import engine, mps

    L, B = engine.lib(), mps._native_builder()
    assert B is not None
    for f in (L.qk_program_size, L.qk_build_run_size, B.qkb_program_size, B.qkb_run_size, B.qkb_result_size):
        f.restype, f.argtypes = C.c_uint32, []
    assert L.qk_program_size() == B.qkb_program_size() == C.sizeof(P.QkProgram)
    assert L.qk_build_run_size() == C.sizeof(P.QkBuildRun)
    assert B.qkb_run_size() == C.sizeof(P.QkbRun) and B.qkb_result_size() == C.sizeof(P.QkbResult)
    assert "qk_build_program" in engine.EXPORTED_SYMBOLS and hasattr(L, "qk_build_program")


def test_a_wrong_size_is_refused_before_anything_else(built):
    from qml_cutensornet_amd import engine, mps

    L, B = engine.lib(), mps._native_builder()
    op, q0, alpha = np.array([0], dtype=np.int8), np.array([0], dtype=np.int32), np.zeros((1, 1))
    for which in ("program", "run"):
        prog, run, h = P.fill_program(1, 2, op, q0, alpha), P.sized(P.QkBuildRun, max_bond=8), C.c_void_p()
        bad = prog if which == "program" else run
        bad.size += 8
        assert L.qk_build_program(None, C.byref(prog), C.byref(run), C.byref(h)) == -1  # QK_EINVAL, with a NULL context
        msg = L.qk_last_error().decode()
        assert msg.startswith("qk_build_program: qk_") and f"{bad.size}" in msg and f"{bad.size - 8}" in msg and h.value is None, msg
    prog, run = P.fill_program(1, 2, op, q0, alpha), P.sized(P.QkBuildRun, max_bond=8)
    assert L.qk_build_program(None, C.byref(prog), C.byref(run), C.byref(h)) == -1 and "null argument" in L.qk_last_error().decode()  # the sizes are right: the context is next
    dims = np.zeros(3, dtype=np.int32)
    for which in range(3):
        structs = [P.fill_program(1, 2, op, q0, alpha), P.sized(P.QkbRun, value_of_zero=1e-16), P.sized(P.QkbResult, dims=dims.ctypes.data)]
        structs[which].size -= 4
        assert B.qkb_simulate_program(*(C.byref(s) for s in structs)) == -8
        msg = B.qkb_last_error().decode()
        assert f"{structs[which].size}" in msg and f"{structs[which].size + 4}" in msg and structs[2].tensors is None, msg
    structs = [P.fill_program(1, 2, op, q0, alpha), P.sized(P.QkbRun, value_of_zero=1e-16), P.sized(P.QkbResult, dims=dims.ctypes.data)]
    assert B.qkb_simulate_program(*(C.byref(s) for s in structs)) == 0 and dims.tolist() == [1, 1, 1] and structs[2].fidelity == 1.0
    B.qkb_free(structs[2].tensors)


def test_fill_program_round_trips_every_field():
    """A program that uses every table: each pointer field is its array's address, each count its leading extent, each scalar itself."""
    rng = np.random.default_rng(3)
    ns, n, n_ops = 3, 5, 7
    arrays = dict(op=rng.integers(0, 12, n_ops).astype(np.int8), q0=rng.integers(0, n, n_ops).astype(np.int32), alpha=rng.standard_normal((ns, n_ops)),
                  mats=rng.standard_normal((ns, 4, 4, 4)) + 0j, mat=rng.integers(0, 4, n_ops).astype(np.int32), kraus=rng.standard_normal((2, 4, 2, 2)) + 0j,
                  n_kraus=np.array([2, 4], dtype=np.int32), kraus2=rng.standard_normal((3, 16, 4, 4)) + 0j, n_kraus2=np.array([1, 16, 4], dtype=np.int32),
                  channel=rng.integers(0, 2, n_ops).astype(np.int32), branch=rng.integers(-1, 2, (ns, n_ops)).astype(np.int32), state_index=np.array([7, 8, 9], dtype=np.uint32),
                  trajectory=np.array([1, 0, 2], dtype=np.uint32), cond_gate=np.full(n_ops, -1, dtype=np.int32), cond_mask=rng.integers(0, 4, n_ops).astype(np.uint32))
    scalars = dict(mats_state_stride=4, branch_state_stride=n_ops, seed=(5 << 32) | 6, first_gate=(1 << 32) - 1)
    p = P.fill_program(ns, n, **arrays, **scalars)
    assert p.size == C.sizeof(P.QkProgram) and (p.n_states, p.n_qubits, p.n_ops) == (ns, n, n_ops)
    assert (p.n_mats, p.n_channels, p.n_channels2) == (4, 2, 3)
    for name, a in arrays.items():
        assert getattr(p, name) == a.ctypes.data, name
    for name, v in scalars.items():
        assert getattr(p, name) == v, name
    assert {f for f, _ in P.QkProgram._fields_} == set(arrays) | set(scalars) | {"size", "n_states", "n_qubits", "n_ops", "n_mats", "n_channels", "n_channels2"}
    for a in arrays.values():  # the addresses are distinct, so no two fields can have been swapped unnoticed
        assert sum(a.ctypes.data == b.ctypes.data for b in arrays.values()) == 1
    bare = P.fill_program(1, n, arrays["op"], arrays["q0"], arrays["alpha"][:1])
    assert (bare.n_mats, bare.n_channels, bare.n_channels2, bare.mats, bare.kraus, bare.cond_gate, bare.state_index) == (0, 0, 0, None, None, None, None)
