"""GPU tests of ``qk_build_program``, the one entry of the device builder: each of the six entries from before it, called through
ctypes with loose arguments, builds bit for bit what the same fields build through the two structs; the launch shape follows the
tables that are present, not the entry; the empty program stays |0...0>.  12 qubits throughout."""
import ctypes as C

import numpy as np
import pytest

from test_conditions_host import teleport_gates
from test_gpu_channels import noisy_12_gates
from test_gpu_channels2 import noisy2_12_gates
from test_matrix_gates_host import brickwork, features, from_gates

pytestmark = pytest.mark.gpu

N = 12
ENTRIES = ["qk_build_mps", "qk_build_mps_scan", "qk_build_mps_gates", "qk_build_mps_channels", "qk_build_mps_channels2", "qk_build_mps_conditions"]


def _ptr(a):
    return None if a is None else a.ctypes.data


def gate_program(circuits, seed=5, first_gate=0, state_index=None, trajectory=None):
    """The arrays of one build call, as ``Context.build_mps`` makes them (by default: state s is named (ns - 1 - s, s % 2))."""
    from qml_cutensornet_amd import engine

    ns = len(circuits)
    return engine._GateProgram("test", circuits, seed, np.arange(ns)[::-1].copy() if state_index is None else state_index, np.arange(ns) % 2 if trajectory is None else trajectory,
                               first_gate)


BUILD_MPS = dict(max_bond=256, budget=max(0.0, 1.0 - (1.0 - 1e-16)))  # the defaults of ``Context.build_mps``


def build_legacy(ctx, entry, gp, max_bond=64, flags=0, cps=None, src=None, src_j=0, budget=1e-16):
    """``gp`` through the entry ``entry`` of before ``qk_build_program``, every argument the entry has spelt out: a ``BuiltScan``."""
    from qml_cutensornet_amd import engine

    level = ENTRIES.index(entry)
    n_ops = int(gp.op.shape[0])
    args = [ctx._h, gp.ns, gp.n, n_ops, _ptr(gp.op), _ptr(gp.q0), _ptr(gp.alpha), budget, 1e-16, max_bond, flags]
    if level >= 1:
        cps = np.array([n_ops], dtype=np.int32) if cps is None else np.ascontiguousarray(cps, dtype=np.int32)
        args += [int(cps.shape[0]), _ptr(cps), None if src is None else src.handle, src_j]
    if level >= 2:
        args += [gp.n_mats, _ptr(gp.mats), gp.stride, _ptr(gp.mat)]
    if level >= 3:
        args += [gp.n_channels, _ptr(gp.kraus), _ptr(gp.n_kraus), _ptr(gp.channel), _ptr(gp.branch), gp.bstride, gp.seed, _ptr(gp.state_index), _ptr(gp.trajectory), gp.first_gate]
    if level >= 4:
        args += [gp.n_channels2, _ptr(gp.kraus2), _ptr(gp.n_kraus2)]
    if level >= 5:
        args += [_ptr(gp.cond_gate), _ptr(gp.cond_mask)]
    h = C.c_void_p()
    engine._check(getattr(engine.lib(), entry)(*args, C.byref(h)), entry)
    return engine.BuiltScan(ctx, h, gp.ns, gp.n)


def build_program(ctx, gp, max_bond=64, flags=0, cps=None, src=None, src_j=0, budget=1e-16, tables=True):
    """The same fields through ``qk_build_program``; ``tables=False`` leaves the channel tables and the condition rows out."""
    from qml_cutensornet_amd import engine
    from qml_cutensornet_amd import program as P

    chan = dict(kraus=gp.kraus, n_kraus=gp.n_kraus, kraus2=gp.kraus2, n_kraus2=gp.n_kraus2, channel=gp.channel, branch=gp.branch, branch_state_stride=gp.bstride,
                cond_gate=gp.cond_gate, cond_mask=gp.cond_mask) if tables else {}
    prog = P.fill_program(gp.ns, gp.n, gp.op, gp.q0, gp.alpha, mats=gp.mats, mat=gp.mat, mats_state_stride=gp.stride, seed=gp.seed, state_index=gp.state_index,
                          trajectory=gp.trajectory, first_gate=gp.first_gate, **chan)
    cps = None if cps is None else np.ascontiguousarray(cps, dtype=np.int32)
    run = P.sized(P.QkBuildRun, flags=flags, trunc_budget=budget, value_of_zero=1e-16, max_bond=max_bond, n_checkpoints=0 if cps is None else int(cps.shape[0]),
                  checkpoints=_ptr(cps), initial=None if src is None else src.handle, initial_snapshot=src_j)
    h = C.c_void_p()
    engine._check(engine.lib().qk_build_program(ctx._h, C.byref(prog), C.byref(run), C.byref(h)), "qk_build_program")
    return engine.BuiltScan(ctx, h, gp.ns, gp.n)


def record(scan):
    """Everything a built handle gives out: per snapshot the downloaded tensors, bond tables, fidelities, log-weights and centres as
    bytes, then the branches, the checkpoints and the launch."""
    out = {"checkpoints": scan.checkpoints, "launch": scan.launch}
    for j in range(len(scan)):
        info = scan.info(j)
        out[j] = [np.ascontiguousarray(t).tobytes() for m in scan.states(j) for t in m.tensors] + [info[k].tobytes() for k in ("dims", "fidelity", "logw", "centre", "branches")]
    return out


def programs():
    """entry -> (circuits, keyword arguments of the build)"""
    import qml_cutensornet_amd as Q
    from oracle import restatement as R

    X = features(3, N, 41)
    ans = Q.KernelStateAnsatz(N, 2, 1.0, Q.entanglement_graph(N, 2))
    plain = [ans.circuit_for_data(x) for x in R.synthetic_features(4, N, 7)]
    tele = from_gates(N, teleport_gates())
    return {
        "qk_build_mps": (plain, {}),
        "qk_build_mps_scan": (plain, dict(cps=[len(plain[0].op) // 2, len(plain[0].op)])),
        "qk_build_mps_gates": ([from_gates(N, brickwork(N, 4, x, seed=17)) for x in X], {}),
        "qk_build_mps_channels": ([from_gates(N, noisy_12_gates(x)) for x in X[:2]], {}),
        "qk_build_mps_channels2": ([from_gates(N, noisy2_12_gates(x)) for x in X[:2]], {}),
        "qk_build_mps_conditions": ([tele, tele.with_branches([1, 0]), tele, tele.with_branches([1, 1]), tele, tele], {}),
    }


@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_with_loose_arguments_builds_the_bits_of_the_program_entry(gpu_ctx, entry):
    circuits, kw = programs()[entry]
    assert 2 <= len(circuits) <= 6 and circuits[0].n_qubits == N
    gp = gate_program(circuits)
    assert (gp.n_mats > 0) == (entry in ENTRIES[2:]) and (gp.n_channels > 0) == (entry in ("qk_build_mps_channels", "qk_build_mps_conditions"))
    assert (gp.n_channels2 > 0) == (entry == "qk_build_mps_channels2") and (gp.cond_gate is not None) == (entry == "qk_build_mps_conditions")
    with build_legacy(gpu_ctx, entry, gp, **kw) as old, build_program(gpu_ctx, gp, **kw) as new:
        want, got = record(old), record(new)
        assert len(old) == len(kw.get("cps", [0])) and old.launch["grid"] == len(circuits)
        assert want == got
        if entry == "qk_build_mps_conditions":
            assert set(old.info(0)["branches"].ravel().tolist()) <= {0, 1} and old.info(0)["branches"][1].tolist() == [1, 0]
        if entry == "qk_build_mps_scan":  # resume from snapshot 0 with the gates that follow it: both entries, the bits of the uninterrupted run
            first = kw["cps"][0]
            import dataclasses

            rest = gate_program([dataclasses.replace(c, op=c.op[first:], q0=c.q0[first:], alpha=c.alpha[first:]) for c in circuits], first_gate=first)
            with build_legacy(gpu_ctx, entry, rest, src=old, src_j=0) as a, build_program(gpu_ctx, rest, cps=[len(rest.op)], src=new, src_j=0) as b:
                assert record(a) == record(b) and record(a)[0] == want[1]


def test_launch_shape_follows_the_tables_present(gpu_ctx):
    """2 states at max_bond 48: 512 threads for a program without channels -- through an entry that could take a channel table, and
    through the program entry with empty tables -- 256 for one with a channel table, and for a plain program resumed from a
    snapshot of that noisy build."""
    X = features(2, N, 3)
    plain = gate_program([from_gates(N, brickwork(N, 2, x, seed=9)) for x in X])
    noisy = gate_program([from_gates(N, brickwork(N, 2, x, seed=9, extras=[("Measure", [6], [])])) for x in X])
    assert plain.n_channels == 0 and noisy.n_channels == 1 and 10 in noisy.op
    with build_legacy(gpu_ctx, "qk_build_mps_channels", plain, max_bond=48) as a, build_program(gpu_ctx, plain, max_bond=48) as b:
        assert a.launch["threads"] == 512 and b.launch["threads"] == 512 and record(a) == record(b)
    with build_program(gpu_ctx, noisy, max_bond=48) as c:
        assert c.launch["threads"] == 256
        with build_program(gpu_ctx, plain, max_bond=48, cps=[len(plain.op)], src=c, src_j=0) as d:
            assert d.launch["threads"] == 256
    with build_legacy(gpu_ctx, "qk_build_mps_channels", noisy, max_bond=48) as e:
        assert e.launch["threads"] == 256


def test_the_empty_program_stays_in_the_zero_state(gpu_ctx):
    from types import SimpleNamespace

    none = np.zeros(0)
    gp = SimpleNamespace(ns=2, n=N, op=none.astype(np.int8), q0=none.astype(np.int32), alpha=np.zeros((2, 0)), mats=None, mat=None, stride=0, seed=0, state_index=None,
                         trajectory=None, first_gate=0)
    with build_legacy(gpu_ctx, "qk_build_mps", gp) as a, build_program(gpu_ctx, gp, tables=False) as b:
        for scan in (a, b):
            assert scan.checkpoints == [0] and len(scan) == 1
            for m in scan.states(0):
                assert m.fidelity == 1.0 and all(t.shape == (1, 2, 1) and t.ravel().tolist() == [1, 0] for t in m.tensors)
        assert record(a) == record(b)
