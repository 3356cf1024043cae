"""Classical control on the host (no GPU): gates conditioned on the recorded branch of an earlier channel gate (``cond_gate``,
``cond_mask``) through the numpy loop and the native host builder -- teleportation and active reset, the exact enumeration of a
program that mixes codes 10 and 11 with conditional unitaries and a conditional channel against dense branch vectors written out
here, the agreement of the two builders on the 12-qubit program of tests/test_gpu_conditions.py, the round trips of the gate-list
forms (``from_gates`` / ``as_tuples``, ``sliced``, ``with_noise``, ``with_branches`` with -2, routing), the rejections, and programs
whose conditions change nothing.  The programs and the list of bad programs of this file are shared with the GPU tests."""
import dataclasses
import math
import re

import numpy as np
import pytest

from test_channels2_host import _matrices
from test_channels_host import BUILDERS, run
from test_matrix_gates_host import apply_dense, brickwork, features, from_gates, haar, mps_vector

SEED = 2025
STATE_INDEX = np.array([0, 0, 1, 1, 2, 2])
TRAJECTORY = np.array([0, 1, 0, 1, 0, 1])
EXTRAS = [("CX", [7, 6], []), ("CZ", [2, 5], [])]


# ---- what a condition means, written out here: the reference of this file
def _values(values):
    return [int(values)] if np.ndim(values) == 0 else [int(v) for v in values]


def dense_branch_vectors(n, gates):
    """Every classical record of an UNROUTED gate list with conditions and the unnormalised vector it leaves: [(record, phi)], the
    record one entry per channel gate in list order (-2: skipped).  A conditional gate acts where the record of the gate it names
    is one of its values; a skipped gate does nothing.  sum |phi><phi| is the density matrix of the program."""
    psi = np.zeros((2,) * n, dtype=complex)
    psi[(0,) * n] = 1.0
    runs = [({}, psi)]
    for pos, g in enumerate(gates):
        name, qubits, params = g[:3]
        cond = g[3] if len(g) == 4 else None
        ms, is_channel = _matrices(name, params)
        nxt = []
        for rec, v in runs:
            if cond is not None and not (rec[cond[0]] >= 0 and rec[cond[0]] in _values(cond[1])):
                nxt.append(({**rec, pos: -2} if is_channel else rec, v))
            elif is_channel:
                nxt.extend(({**rec, pos: b}, apply_dense(v, m, list(qubits))) for b, m in enumerate(ms))
            else:
                nxt.append((rec, apply_dense(v, ms[0], list(qubits))))
        runs = nxt
    return [(tuple(rec[p] for p in sorted(rec)), v.reshape(-1)) for rec, v in runs]


def runs_and_skips(c, branches):
    """Per conditional gate of the program (ascending position): did it run in the trajectory that recorded ``branches``?"""
    col = np.cumsum(np.isin(c.op, (10, 11))) - 1  # the column of a channel gate in the record
    out = []
    for i in np.flatnonzero(c.cond_gate >= 0):
        b = int(branches[col[c.cond_gate[i]]])
        out.append(b >= 0 and bool((int(c.cond_mask[i]) >> b) & 1))
    return out


def bloch_of(v, n, q):
    """(<X>, <Y>, <Z>) of qubit q of the normalised vector v."""
    t = np.moveaxis(np.asarray(v).reshape((2,) * n), q, 0).reshape(2, -1)
    rho = t @ t.conj().T
    return np.array([2 * rho[0, 1].real, -2 * rho[0, 1].imag, (rho[0, 0] - rho[1, 1]).real])  # rho = (1 + r . sigma) / 2


# ---- teleportation and reset
TELE_A, TELE_B = 0.37, 0.81


def teleport_gates(conditional=True):
    """3 qubits: Ry(a) Rz(b) on qubit 0, a Bell pair on (1, 2), the Bell measurement of (0, 1) as CX, H and two Measure gates (list
    positions 6 and 7), then X on qubit 2 if m1 = 1 and Z on qubit 2 if m0 = 1."""
    gates = [("Ry", [0], [TELE_A]), ("Rz", [0], [TELE_B]), ("H", [1], []), ("CX", [1, 2], []), ("CX", [0, 1], []), ("H", [0], []), ("Measure", [0], []), ("Measure", [1], [])]
    return gates + ([("X", [2], [], (7, 1)), ("Z", [2], [], (6, [1]))] if conditional else [])


def teleported_bloch():
    return bloch_of(mps_vector(run(from_gates(1, [("Ry", [0], [TELE_A]), ("Rz", [0], [TELE_B])]), "numpy")), 1, 0)


RESET_GATES = [("H", [0], []), ("Measure", [0], []), ("X", [0], [], (1, 1))]


@pytest.mark.parametrize("builder", BUILDERS)
def test_teleportation(built, builder):
    c, plain = from_gates(3, teleport_gates()), from_gates(3, teleport_gates(False))
    assert c.cond_gate.tolist() == [-1] * 8 + [7, 6] and c.cond_mask.tolist() == [0] * 8 + [2, 2] and plain.cond_gate is None
    want = teleported_bloch()
    assert np.abs(want).min() > 0.05  # a generic vector: every correction shows
    for m0 in (0, 1):
        for m1 in (0, 1):
            m = run(c.with_branches([m0, m1]), builder)
            assert m.branches.tolist() == [m0, m1]
            assert np.abs(bloch_of(mps_vector(m), 3, 2) - want).max() < 1e-12 and abs(m.logw - math.log(0.25)) < 1e-12
            bare = bloch_of(mps_vector(run(plain.with_branches([m0, m1]), builder)), 3, 2)
            assert (np.abs(bare - want).max() > 0.05) == ((m0, m1) != (0, 0))  # without the corrections only outcome 00 teleports
    seen = set()
    for t in range(12):
        m = run(c, builder, seed=SEED, state_index=1, trajectory=t)
        seen.add(tuple(m.branches.tolist()))
        assert np.abs(bloch_of(mps_vector(m), 3, 2) - want).max() < 1e-12 and abs(m.logw - math.log(0.25)) < 1e-12
    assert len(seen) >= 3


@pytest.mark.parametrize("builder", BUILDERS)
def test_active_reset(built, builder):
    c = from_gates(1, RESET_GATES)
    seen = set()
    for t in range(16):
        m = run(c, builder, seed=SEED, trajectory=t)
        seen.add(int(m.branches[0]))
        assert abs(bloch_of(mps_vector(m), 1, 0)[2] - 1) < 1e-14
    assert seen == {0, 1}


# ---- exact enumeration
def enum_gates():
    """n = 5: codes 10 and 11 with conditional unitaries of every arity, a conditional channel of each code, a routed conditional
    gate and a condition on a conditional gate.  Channel gates at list positions 4, 7, 10, 12."""
    u = haar(np.random.default_rng(3), 4)
    return [("H", [0], []), ("CX", [0, 1], []), ("Ry", [2], [0.3]), ("CX", [1, 2], []),
            ("AmplitudeDamping", [1], [0.4]),  # 4
            ("XXPhase", [2, 3], [0.4]), ("Ry", [4], [0.6]),
            ("Measure2q", [3, 4], []),  # 7
            ("X", [0], [], (4, 1)), ("Unitary2q", [1, 2], [u], (7, [1, 2])),
            ("Depolarizing", [2], [0.5], (7, [0, 3])),  # 10: a conditional channel
            ("CX", [0, 3], [], (10, [1, 2, 3])),  # a routed gate, conditioned on a conditional gate
            ("CorrelatedPhaseFlip", [3, 2], [0.3], (4, 0)),  # 12: a conditional two-qubit channel, qubits reversed
            ("Rz", [3], [0.7], (12, 1)), ("YYPhase", [0, 1], [0.2]), ("Ry", [4], [0.2], (10, []))]


@pytest.mark.parametrize("builder", BUILDERS)
def test_exact_enumeration_with_conditions(built, builder):
    n, gates = 5, enum_gates()
    c = from_gates(n, gates)
    assert c.op[np.isin(c.op, (10, 11))].tolist() == [10, 11, 10, 11] and int(np.count_nonzero(c.cond_gate >= 0)) == 6 + 5  # the routed CX is five ops
    want, rho, total, skipped = np.zeros((2 ** n, 2 ** n), dtype=complex), np.zeros((2 ** n, 2 ** n), dtype=complex), 0.0, 0
    for rec, phi in dense_branch_vectors(n, gates):
        want += np.outer(phi, phi.conj())
        if np.vdot(phi, phi).real < 1e-20:
            continue  # an impossible record: the builders refuse to force it
        m = run(c.with_branches(list(rec)), builder)
        assert m.branches.tolist() == list(rec) and abs(m.fidelity - 1) < 1e-12
        v = mps_vector(m)
        assert abs(np.vdot(v, v).real - 1) < 1e-12
        rho += math.exp(m.logw) * np.outer(v, v.conj())
        total += math.exp(m.logw)
        skipped += -2 in rec
    assert skipped > 0 and abs(np.trace(want).real - 1) < 1e-13
    assert abs(total - 1) < 1e-10 and np.abs(rho - want).max() < 1e-10


# ---- the 12-qubit program of the GPU tests
SPLIT_12 = 3  # brickwork layers in front of the measurements
def cond_12_gates(x, conditional=True):
    """n = 12: the six-layer Haar brickwork of tests/test_gpu_channels.py; behind its third layer a Measure (A) and a Measure2q (B)
    and conditional gates of every kind: a named constant, a data-dependent Rz, XXPhase, Unitary2q, a code-10 channel (C) and a
    code-11 channel (D), a gate on non-adjacent qubits, and gates conditioned on the conditional channels.  ``conditional=False``:
    the same gates with every condition removed."""
    n = 12
    first, rest = brickwork(n, SPLIT_12, x, seed=17), brickwork(n, 6, x, seed=17, extras=EXTRAS)
    u = haar(np.random.default_rng(29), 4)
    A = len(first)
    B, C, D = A + 1, A + 6, A + 7
    mid = [("Measure", [5], []), ("Measure2q", [6, 7], []),
           ("X", [4], [], (A, 1)), ("Rz", [2], [float(x[2])], (A, 0)), ("XXPhase", [8, 9], [0.3], (B, [1, 2])), ("Unitary2q", [1, 0], [u], (B, [0, 3])),
           ("Depolarizing", [6], [0.9], (A, 1)), ("Measure2q", [4, 5], [], (B, [2, 3])),
           ("CX", [3, 7], [], (B, [0, 1])), ("Z", [5], [], (D, [1, 3])), ("YYPhase", [2, 3], [0.4], (C, [1, 2, 3]))]
    if not conditional:
        mid = [g[:3] for g in mid]
    return rest[: len(first)] + mid + rest[len(first):]


def cond_12_circuits():
    return [from_gates(12, cond_12_gates(x)) for x in features(3, 12, 41) for _ in range(2)]


def test_numpy_and_native_builder_agree_on_the_12_qubit_program(built):
    circuits = cond_12_circuits()
    c0 = circuits[0]
    assert sorted(set(c0.op[c0.cond_gate >= 0].tolist())) == [1, 2, 3, 6, 8, 9, 10, 11]
    ran, worst, bond = [], np.inf, 0
    for c, s, t in zip(circuits, STATE_INDEX, TRAJECTORY):
        a, margin = run(c, "numpy", seed=SEED, state_index=int(s), trajectory=int(t), margin=True)
        b, margin_b = run(c, "native", seed=SEED, state_index=int(s), trajectory=int(t), margin=True)
        worst, bond = min(worst, margin_b), max(bond, b.max_bond())
        assert np.array_equal(a.branches, b.branches) and abs(a.logw - b.logw) < 1e-10 and abs(margin - margin_b) < 1e-9
        assert abs(abs(np.vdot(mps_vector(a), mps_vector(b))) ** 2 - 1) < 1e-10
        ran.append(runs_and_skips(c, b.branches))
    # what the GPU tests rest on: no draw of the host at a threshold, bond 64, every conditional gate both run and skipped
    assert worst >= 1e-6 and bond == 64
    ran = np.array(ran)
    assert ran.any(axis=0).all() and (~ran).any(axis=0).all()


# ---- round trips
@pytest.mark.parametrize("builder", BUILDERS)
def test_gate_lists_round_trip(built, builder):
    n, gates = 5, enum_gates()
    c = from_gates(n, gates)
    tuples = c.as_tuples()
    assert len(tuples) == c.n_gates and [len(t) for t in tuples] == [4 if g >= 0 else 3 for g in c.cond_gate.tolist()]
    back = from_gates(n, tuples)
    assert np.array_equal(back.cond_gate, c.cond_gate) and np.array_equal(back.cond_mask, c.cond_mask) and np.array_equal(back.op, c.op)
    a, b = run(c, builder, seed=4, state_index=2), run(back, builder, seed=4, state_index=2)
    assert a.logw == b.logw and np.array_equal(a.branches, b.branches) and all(np.array_equal(x, y) for x, y in zip(a.tensors, b.tensors))
    # a condition on a forced gate: the list holds Project / Project2q (one branch), the condition reads [0] or []
    rec = [0, 2, -2, 1]  # the damping forced to 0, the Measure2q to 2: the Depolarizing (left drawn) is skipped, the flip runs, forced to 1
    forced = c.with_branches([0, 2, -1, 1])
    ft = forced.as_tuples()
    assert [t[0] for t in ft if t[0].startswith(("Kraus", "Project"))] == ["Project", "Project2q", "Kraus1q", "Project2q"]
    # (program positions: the X 8, the Unitary2q 9, the Depolarizing 10, the routed CX 11 .. 15, the flip 16, the Rz 17)
    assert ft[8][0] == "Unitary1q" and ft[8][3] == (4, []) and ft[9][3] == (7, [0]) and ft[10][0] == "Kraus1q" and ft[10][3] == (7, [])
    assert ft[13][3] == (10, [1, 2, 3]) and ft[16][0] == "Project2q" and ft[16][3] == (4, [0]) and ft[17][0] == "Rz" and ft[17][3] == (16, [0])
    again = from_gates(n, ft)
    a, b = run(forced, builder, seed=4), run(again, builder, seed=4)
    assert a.branches.tolist() == rec and b.branches.tolist() == [0, 0, -2, 0]
    assert a.logw == b.logw and all(np.array_equal(x, y) for x, y in zip(a.tensors, b.tensors))
    # with_branches with -2 keeps the program's own entry: the replay of a record reproduces the skips
    skips = 0
    for si in range(6):
        m = run(c, builder, seed=4, state_index=si)
        replay = run(c.with_branches(m.branches), builder, seed=99)
        assert np.array_equal(replay.branches, m.branches) and replay.logw == m.logw and all(np.array_equal(x, y) for x, y in zip(replay.tensors, m.tensors))
        skips += -2 in m.branches
    assert skips > 0
    kept = forced.with_branches([-2, -2, -2, -2])
    assert np.array_equal(kept.branch, forced.branch) and np.array_equal(kept.cond_gate, c.cond_gate)


def test_sliced_shifts_and_refuses(built):
    c = from_gates(5, enum_gates())
    first = int(np.flatnonzero(c.op == 10)[0])  # the AmplitudeDamping
    tail = c.sliced(first, c.n_gates)
    assert np.array_equal(tail.cond_gate, np.where(c.cond_gate[first:] >= 0, c.cond_gate[first:] - first, -1)) and np.array_equal(tail.cond_mask, c.cond_mask[first:])
    with pytest.raises(ValueError, match=rf"gate {first + 4} is conditioned on gate {first}, which lies in front of the slice"):
        c.sliced(first + 1, c.n_gates)  # the X that reads the damping
    head = c.sliced(0, first + 3)
    assert head.cond_gate is not None and head.cond_gate.max() == -1
    plain = from_gates(3, [("H", [0], []), ("CX", [0, 1], [])])
    assert plain.sliced(1, 2).cond_gate is None


@pytest.mark.parametrize("builder", BUILDERS)
def test_a_routed_conditional_gate_is_skipped_as_a_whole(built, builder):
    n = 5
    head = [("H", [0], []), ("CX", [0, 1], []), ("Ry", [3], [0.7]), ("Measure", [2], [])]  # qubit 2 is |0>: the outcome is 0
    c = from_gates(n, head + [("CX", [0, 4], [], (3, 1)), ("Depolarizing2q", [4, 1], [0.3], (3, 1))])
    assert c.op.tolist()[4:] == [3, 3, 3, 9, 3, 3, 3] + [3, 3, 11, 3, 3] and c.cond_gate.tolist()[4:] == [3] * 12 and c.cond_mask.tolist()[4:] == [2] * 12
    m, bare = run(c, builder, seed=1), run(from_gates(n, head), builder, seed=1)
    assert m.branches.tolist() == [0, -2] and m.logw == bare.logw and all(np.array_equal(x, y) for x, y in zip(m.tensors, bare.tensors))
    ran = run(from_gates(n, head[:3] + [("X", [2], []), ("Measure", [2], []), ("CX", [0, 4], [], (4, 1)), ("Depolarizing2q", [4, 1], [0.3], (4, 1)), ("Z", [0], [], (6, [0]))]),
              builder, seed=1)
    assert ran.branches[0] == 1 and ran.branches[1] >= 0 and ran.max_bond() >= 2
    # a condition names the core op of a routed channel gate
    far = from_gates(n, head + [("Measure2q", [0, 3], []), ("X", [4], [], (4, [1, 3]))])
    assert far.op.tolist()[4:] == [3, 3, 11, 3, 3, 8] and far.cond_gate.tolist()[-1] == 6


def test_with_noise_remaps_conditions(built):
    from qml_cutensornet_amd.engine import with_noise

    gates = [("H", [0], []), ("CX", [0, 1], []), ("Measure", [1], []), ("X", [0], [], (2, 1)), ("XXPhase", [0, 2], [0.3], (2, [0]))]
    noisy = with_noise(gates, "BitFlip", [0.1])
    assert [(g[0], g[1]) for g in noisy] == [("H", [0]), ("BitFlip", [0]), ("CX", [0, 1]), ("BitFlip", [0]), ("BitFlip", [1]), ("Measure", [1]), ("X", [0]), ("BitFlip", [0]),
                                            ("XXPhase", [0, 2]), ("BitFlip", [0]), ("BitFlip", [2])]
    assert [g[3] for g in noisy if len(g) == 4] == [(5, 1), (5, 1), (5, [0]), (5, [0]), (5, [0])]  # the channel behind a conditional gate takes its condition
    pair = with_noise(gates, "Depolarizing2q", [0.1], after="two_qubit")
    assert [(g[0],) + tuple(g[3:]) for g in pair] == [("H",), ("CX",), ("Depolarizing2q",), ("Measure",), ("X", (3, 1)), ("XXPhase", (3, [0])), ("Depolarizing2q", (3, [0]))]
    c = from_gates(3, noisy)
    at = int(np.flatnonzero(c.op == 10)[3])  # the Measure
    assert set(c.cond_gate[c.cond_gate >= 0].tolist()) == {at}
    for t in range(4):
        m = run(c, "native", seed=3, trajectory=t)
        skipped = m.branches == -2
        assert skipped.tolist() == ([False] * 4 + [False, True, True] if m.branches[3] == 1 else [False] * 4 + [True, False, False])


def test_templates_take_conditions(built):
    import qml_cutensornet_amd as Q

    ans = Q.CircuitAnsatz(3, [("H", [0], None), ("XXPhase", [0, 1], (0.4, (0, 1.0, -1.0))), ("Measure", [1], None), ("Unitary1q", [0], np.array([[0, 1], [1, 0]]), (2, 1)),
                             ("Rz", [2], (1.0, (2, 0.0, 1.0)), (2, [0, 1])), ("ZZPhase", [0, 2], 0.3, (2, 0))])
    p = ans.ansatz_circ
    assert p.cond_gate.tolist() == [-1, -1, -1, 2, 2, 2, 2, 2] and p.cond_mask.tolist() == [0, 0, 0, 2, 3, 1, 1, 1]
    a, b = ans.circuit_for_data(np.array([0.1, 0.2, 0.3])), ans.circuit_for_data(np.array([0.4, 0.5, 0.6]))
    assert a.cond_gate is b.cond_gate and a.cond_mask is b.cond_mask
    gl = from_gates(3, [("H", [0], []), ("XXPhase", [0, 1], [0.4 * 0.9]), ("Measure", [1], []), ("X", [0], [], (2, 1)), ("Rz", [2], [0.3], (2, [0, 1])), ("ZZPhase", [0, 2], [0.3], (2, 0))])
    for t in range(3):
        x, y = run(a, "native", seed=2, trajectory=t), run(gl, "native", seed=2, trajectory=t)
        assert np.array_equal(x.branches, y.branches) and abs(abs(np.vdot(mps_vector(x), mps_vector(y))) ** 2 - 1) < 1e-12
    assert Q.CircuitAnsatz(2, [("H", [0], None)]).ansatz_circ.cond_gate is None
    for bad in ([("H", [0], [], (0, 1))], [("H", [0], []), ("X", [0], [], (0, 1))], [("Measure", [0], []), ("X", [0], [], (0, [32]))], [("Measure", [0], []), ("X", [0], [], 0)],
                [("Measure", [0], []), ("X", [0], [], (1, 0))]):
        with pytest.raises(ValueError, match="gate [01]"):
            from_gates(2, bad)


# ---- rejections
def _ok_cond_program():
    """n = 4: channel gates at positions 2 (Measure, two branches) and 4 (Measure2q, four); conditional gates at 3, 5, 6."""
    return from_gates(4, [("H", [0], []), ("CX", [0, 1], []), ("Measure", [1], []), ("X", [2], [], (2, 1)), ("Measure2q", [2, 3], [], (2, [0, 1])), ("Rz", [0], [0.3], (4, [1, 3])),
                          ("XXPhase", [1, 2], [0.2], (4, 2))])


def bad_condition_programs():
    """[(label, circuit, text the error must hold)]; entry 0 is the good program."""
    ok = _ok_cond_program()
    R = dataclasses.replace

    def arr(a, i, v):
        a = np.array(a, copy=True)
        a[i] = v
        return a

    plain = from_gates(4, [("H", [0], []), ("CX", [0, 1], []), ("Rz", [1], [0.2])])
    return [
        ("ok", ok, ""),
        ("rows without a channel table", R(plain, cond_gate=np.array([-1, -1, 1], dtype=np.int32), cond_mask=np.array([0, 0, 1], dtype=np.uint32)), "gate 0: .*channel table"),
        ("cond_gate below -1", R(ok, cond_gate=arr(ok.cond_gate, 1, -2)), "gate 1: condition on gate -2"),
        ("a condition on itself", R(ok, cond_gate=arr(ok.cond_gate, 5, 5)), "gate 5: condition on gate 5"),
        ("a condition on a later gate", R(ok, cond_gate=arr(ok.cond_gate, 3, 4)), "gate 3: condition on gate 4"),
        ("a condition on a gate that is no channel", R(ok, cond_gate=arr(ok.cond_gate, 6, 3)), "gate 6: condition on gate 3, which is no channel gate"),
        ("a mask bit above the two branches", R(ok, cond_mask=arr(ok.cond_mask, 3, 4)), "gate 3: condition mask"),
        ("a mask bit above the four branches", R(ok, cond_mask=arr(ok.cond_mask, 6, 1 << 4)), "gate 6: condition mask"),
        ("no cond_mask", R(ok, cond_mask=None), "cond_mask"),
    ]


N_BAD_CONDITIONS = 8


@pytest.mark.parametrize("builder", BUILDERS)
def test_rejections_name_the_gate(built, builder):
    progs = bad_condition_programs()
    assert len(progs) == N_BAD_CONDITIONS + 1
    assert run(progs[0][1], builder).branches.shape == (2,)
    for label, c, text in progs[1:]:
        with pytest.raises(ValueError, match=text):
            run(c, builder)
    with pytest.raises(ValueError, match=progs[2][2]):
        progs[2][1].as_tuples()
    never = dataclasses.replace(progs[0][1], cond_mask=np.zeros_like(progs[0][1].cond_mask))  # mask 0, "never", is valid
    assert run(never, builder, seed=1).branches[1] == -2


def test_the_native_entry_returns_minus_8(built):
    """``qkb_simulate_program`` itself: -8 with the gate named, before a gate is applied."""
    import ctypes as C

    from qml_cutensornet_amd import mps
    from qml_cutensornet_amd import program as P

    lib = mps._native_builder()
    assert lib is not None
    for label, c, text in bad_condition_programs()[2:]:
        op, q0, alpha = np.ascontiguousarray(c.op, dtype=np.int8), np.ascontiguousarray(c.q0, dtype=np.int32), np.ascontiguousarray(c.alpha, dtype=np.float64)
        kraus, nk = np.ascontiguousarray(c.kraus, dtype=np.complex128), np.ascontiguousarray(c.n_kraus, dtype=np.int32)
        kraus2, nk2 = np.ascontiguousarray(c.kraus2, dtype=np.complex128), np.ascontiguousarray(c.n_kraus2, dtype=np.int32)
        channel, branch = np.ascontiguousarray(c.channel, dtype=np.int32), np.ascontiguousarray(c.branch, dtype=np.int32)
        mats, mat = np.ascontiguousarray(c.mats, dtype=np.complex128), np.ascontiguousarray(c.mat, dtype=np.int32)
        cg = np.ascontiguousarray(c.cond_gate, dtype=np.int32)
        cm = None if c.cond_mask is None else np.ascontiguousarray(c.cond_mask, dtype=np.uint32)
        dims = np.full(5, -7, dtype=np.int32)
        prog = P.fill_program(1, 4, op, q0, alpha, mats=mats, mat=mat, kraus=kraus, n_kraus=nk, kraus2=kraus2, n_kraus2=nk2, channel=channel, branch=branch, cond_gate=cg, cond_mask=cm)
        run, res = P.sized(P.QkbRun, trunc_budget=0.0, value_of_zero=1e-16), P.sized(P.QkbResult, dims=dims.ctypes.data)
        rc = lib.qkb_simulate_program(C.byref(prog), C.byref(run), C.byref(res))
        assert rc == -8 and res.tensors is None and dims.tolist() == [-7] * 5, label
        assert re.search(text, lib.qkb_last_error().decode()), (label, lib.qkb_last_error())


# ---- conditions that change nothing
@pytest.mark.parametrize("builder", BUILDERS)
def test_programs_whose_conditions_change_nothing_are_bit_equal(built, builder):
    from test_channels2_host import _noisy2_8

    _, _, noisy = _noisy2_8()
    rows = dataclasses.replace(noisy, cond_gate=np.full(noisy.op.shape, -1, dtype=np.int32), cond_mask=np.zeros(noisy.op.shape, dtype=np.uint32))
    kw = dict(seed=11, state_index=3, trajectory=2, max_bond=6)
    a, b = run(noisy, builder, **kw), run(rows, builder, **kw)
    assert a.fidelity == b.fidelity and a.logw == b.logw and np.array_equal(a.branches, b.branches) and all(np.array_equal(x, y) for x, y in zip(a.tensors, b.tensors))
    # conditions that all hold: full masks on forced gates
    gates = enum_gates()
    bare = from_gates(5, [g[:3] for g in gates]).with_branches([1, 2, 3, 0])
    c = from_gates(5, gates)
    full = dataclasses.replace(bare, cond_gate=c.cond_gate, cond_mask=full_masks(c))
    a, b = run(bare, builder), run(full, builder)
    assert a.branches.tolist() == b.branches.tolist() == [1, 2, 3, 0]
    assert a.fidelity == b.fidelity and a.logw == b.logw and all(np.array_equal(x, y) for x, y in zip(a.tensors, b.tensors))


def full_masks(c):
    """Per conditional gate the mask of every branch of the channel gate it names."""
    mask = np.zeros(c.n_gates, dtype=np.uint32)
    for i in np.flatnonzero(c.cond_gate >= 0):
        g = int(c.cond_gate[i])
        mask[i] = (1 << int((c.n_kraus if c.op[g] == 10 else c.n_kraus2)[c.channel[g]])) - 1
    return mask


def test_seedless_paths_take_conditions_on_forced_gates(built):
    import qml_cutensornet_amd as Q
    from qml_cutensornet_amd import mps

    forced = [("H", [0], None), ("XXPhase", [0, 1], 0.3), ("PostSelect", [1], [1]), ("X", [0], None, (2, 1)), ("Z", [1], None, (2, 0))]
    drawn = forced[:2] + [("Measure", [1], None)] + forced[3:]
    X = np.array([[0.1, 0.2], [0.3, 0.4]])
    states, _ = mps.simulate_many([Q.CircuitAnsatz(2, forced).circuit_for_data(x) for x in X], workers=1)
    assert all(m.branches.tolist() == [1] for m in states)
    with pytest.raises(ValueError, match="drawn Kraus channels"):
        mps.simulate_many([Q.CircuitAnsatz(2, drawn).circuit_for_data(x) for x in X], workers=1)
