"""Kraus channels and post-selection on the host (no GPU): op code 10 through both host builders against a dense density matrix and
dense state-vector trajectories written out here, the named channels, forced branches and replay, the Philox stream of the draws,
the agreement of the two builders' draws (behind a margin), the rejections, and programs without channels through the new entry.
The dense simulators, the circuits and the list of bad programs of this file are shared with tests/test_gpu_channels.py."""
import dataclasses
import math
import pickle

import numpy as np
import pytest

from test_matrix_gates_host import NAMED, apply_dense, brickwork, dense_state, features, from_gates, gate_matrix, mps_vector

CHANNELS = ("Kraus1q", "Project", "Measure", "PostSelect", "AmplitudeDamping", "PhaseDamping", "Depolarizing", "BitFlip", "PhaseFlip")
_I2, _X, _Y, _Z = np.eye(2, dtype=complex), np.array(NAMED["X"], dtype=complex), np.array(NAMED["Y"], dtype=complex), np.array(NAMED["Z"], dtype=complex)
_P = [np.diag([1.0, 0.0]).astype(complex), np.diag([0.0, 1.0]).astype(complex)]


def kraus_of(name, params):
    """The Kraus matrices of a named channel, written out here: the reference of this file, independent of the table under test."""
    if name in ("Kraus1q", "Project"):
        k = np.asarray(params[0], dtype=complex)
        return list(k) if k.ndim == 3 else [k]
    if name in ("Measure", "PostSelect"):
        return list(_P)
    p = float(params[0])
    if name == "AmplitudeDamping":
        return [np.array([[1, 0], [0, math.sqrt(1 - p)]], dtype=complex), np.array([[0, math.sqrt(p)], [0, 0]], dtype=complex)]
    if name == "PhaseDamping":
        return [np.array([[1, 0], [0, math.sqrt(1 - p)]], dtype=complex), np.array([[0, 0], [0, math.sqrt(p)]], dtype=complex)]
    if name == "Depolarizing":
        return [math.sqrt(1 - 0.75 * p) * _I2, math.sqrt(p / 4) * _X, math.sqrt(p / 4) * _Y, math.sqrt(p / 4) * _Z]
    return [math.sqrt(1 - p) * _I2, math.sqrt(p) * (_X if name == "BitFlip" else _Z)]


def dense_rho(n, gates):
    """The density matrix of an unrouted gate list with channels applied as Kraus maps, (2^n, 2^n)."""
    d = 2 ** n
    rho = np.zeros((d, d), dtype=complex)
    rho[0, 0] = 1.0

    def left(r, m, qubits):  # m on the row index of r
        return apply_dense(r.reshape((2,) * n + (d,)), m, qubits).reshape(d, d)

    for name, qubits, params in gates:
        ms = kraus_of(name, params) if name in CHANNELS else [gate_matrix(name, params[0] if params is not None and len(params) else None)]
        rho = sum(left(left(rho, m, list(qubits)).conj().T, m, list(qubits)).conj().T for m in ms)
    return rho


def dense_trajectory(n, gates, branches):
    """The state vector of one trajectory: channel gate j applies its Kraus matrix ``branches[j]`` and renormalises.  Returns
    (psi, logw) with logw the sum of the logs of the branch probabilities."""
    psi = np.zeros((2,) * n, dtype=complex)
    psi[(0,) * n] = 1.0
    logw, j = 0.0, 0
    for name, qubits, params in gates:
        if name in CHANNELS:
            psi = apply_dense(psi, kraus_of(name, params)[int(branches[j])], list(qubits))
            p = float(np.vdot(psi, psi).real)
            psi = psi / math.sqrt(p)
            logw += math.log(p)
            j += 1
        else:
            psi = apply_dense(psi, gate_matrix(name, params[0] if params is not None and len(params) else None), list(qubits))
    assert j == len(branches)
    return psi.reshape(-1), logw


def run(c, builder, **kw):
    from qml_cutensornet_amd import mps

    if builder == "numpy":
        return mps._simulate(c, 1.0, 1e-16, kw.pop("max_bond", None), None, **kw)
    return mps.simulate_native(c, 1.0, 1e-16, kw.pop("max_bond", None), **kw)


BUILDERS = ["numpy", "native"]

# n = 6: a short entangling circuit with two AmplitudeDamping(0.3) gates -- the first on qubit 1 while the orthogonality centre sits
# on (4, 5), the second on the last qubit
ENUM_GATES = [("H", [0], []), ("CX", [0, 1], []), ("Ry", [2], [0.3]), ("CX", [1, 2], []), ("XXPhase", [2, 3], [0.4]), ("CX", [3, 4], []), ("ZZPhase", [4, 5], [0.3]),
              ("Rx", [5], [0.7]), ("XXPhase", [4, 5], [0.6]), ("AmplitudeDamping", [1], [0.3]), ("CX", [2, 3], []), ("Ry", [5], [0.4]), ("AmplitudeDamping", [5], [0.3]),
              ("YYPhase", [0, 1], [0.2])]


def noisy_brickwork(n, layers, x, seed):
    """The Haar brickwork of tests/test_matrix_gates_host.py with AmplitudeDamping(0.05) behind every two-qubit gate and a Measure in
    mid-chain after the first half of it."""
    from qml_cutensornet_amd.engine import with_noise

    gates = with_noise(brickwork(n, layers, x, seed=seed), "AmplitudeDamping", [0.05], after="two_qubit")
    half = len(gates) // 2
    return gates[:half] + [("Measure", [n // 2], [])] + gates[half:]


@pytest.mark.parametrize("builder", BUILDERS)
def test_exact_enumeration_of_two_damping_gates(built, builder):
    n = 6
    c = from_gates(n, ENUM_GATES)
    assert c.op.tolist().count(10) == 2 and c.n_channel_gates == 2 and c.q0[c.op == 10].tolist() == [1, 5]
    want = dense_rho(n, ENUM_GATES)
    assert abs(np.trace(want).real - 1) < 1e-13
    rho, total = np.zeros_like(want), 0.0
    for b0 in (0, 1):
        for b1 in (0, 1):
            m = run(c.with_branches([b0, b1]), builder)
            assert m.branches.tolist() == [b0, b1] and abs(m.fidelity - 1) < 1e-12
            v = mps_vector(m)
            assert abs(np.vdot(v, v).real - 1) < 1e-12  # back at norm 1
            rho += math.exp(m.logw) * np.outer(v, v.conj())
            total += math.exp(m.logw)
    assert abs(total - 1) < 1e-12
    assert np.abs(rho - want).max() < 1e-12


@pytest.mark.parametrize("builder", BUILDERS)
def test_named_channels_on_small_states(built, builder):
    g = 0.3
    c = from_gates(2, [("X", [1], []), ("AmplitudeDamping", [1], [g])])
    for b, ket, logw in ((1, [1, 0, 0, 0], math.log(g)), (0, [0, 1, 0, 0], math.log(1 - g))):
        m = run(c.with_branches([b]), builder)
        assert np.abs(np.abs(mps_vector(m)) - np.array(ket)).max() < 1e-15 and abs(m.logw - logw) < 1e-15
    # PostSelect on a GHZ state built with CX: probability 1/2 and the collapsed product state
    n = 5
    ghz = [("H", [0], [])] + [("CX", [q, q + 1], []) for q in range(n - 1)]
    for bit in (0, 1):
        m = run(from_gates(n, ghz + [("PostSelect", [2], [bit])]), builder)
        v = mps_vector(m)
        assert abs(m.logw - math.log(0.5)) < 1e-14 and m.branches.tolist() == [bit]
        assert abs(abs(v[-1 if bit else 0]) - 1) < 1e-14 and abs(np.vdot(v, v).real - 1) < 1e-14
    # a forced Pauli branch of Depolarizing is the named constant gate
    p = 0.2
    prep = [("Ry", [0], [0.37]), ("Rz", [0], [0.21]), ("Ry", [1], [-0.58]), ("Rz", [1], [0.44]), ("XXPhase", [0, 1], [0.3])]
    for b, name in ((1, "X"), (2, "Y"), (3, "Z")):
        m = run(from_gates(2, prep + [("Depolarizing", [1], [p])]).with_branches([b]), builder)
        assert np.abs(mps_vector(m) - dense_state(2, prep + [(name, [1], [])])).max() < 1e-13 and abs(m.logw - math.log(p / 4)) < 1e-13
    # Project takes any finite matrix, Kraus1q a list; PhaseDamping, BitFlip and PhaseFlip against the dense density matrix
    M = np.array([[0.9, 0.1j], [0.2, 0.4]])
    m = run(from_gates(2, prep + [("Project", [0], [M])]), builder)
    psi, logw = dense_trajectory(2, prep + [("Project", [0], [M])], [0])
    assert np.abs(mps_vector(m) - psi).max() < 1e-13 and abs(m.logw - logw) < 1e-13
    for name, params in (("PhaseDamping", [0.4]), ("BitFlip", [0.1]), ("PhaseFlip", [0.25]), ("Kraus1q", [kraus_of("AmplitudeDamping", [0.6])]), ("Measure", [])):
        gates = prep + [(name, [0], params), ("CX", [0, 1], [])]
        c = from_gates(2, gates)
        k = len(kraus_of(name, params))
        rho = np.zeros((4, 4), dtype=complex)
        for b in range(k):
            r = run(c.with_branches([b]), builder)
            rho += math.exp(r.logw) * np.outer(mps_vector(r), mps_vector(r).conj())
        assert np.abs(rho - dense_rho(2, gates)).max() < 1e-13, name


def _noisy_8(seed_x=3):
    n = 8
    gates = noisy_brickwork(n, 4, features(1, n, seed_x)[0], seed=5)
    return n, gates, from_gates(n, gates)


@pytest.mark.parametrize("builder", BUILDERS)
def test_drawn_trajectories_match_dense_trajectories_and_replay(built, builder):
    n, gates, c = _noisy_8()
    assert c.n_channel_gates == 2 * sum(g[0] == "Unitary2q" for g in gates) + 1
    for si, tr in ((0, 0), (0, 1), (5, 0)):
        m = run(c, builder, seed=11, state_index=si, trajectory=tr)
        assert m.branches.shape == (c.n_channel_gates,) and m.branches.min() >= 0
        psi, logw = dense_trajectory(n, gates, m.branches)
        assert abs(abs(np.vdot(psi, mps_vector(m))) ** 2 - 1) < 1e-10
        assert abs(m.logw - logw) < 1e-12
        again = run(c, builder, seed=11, state_index=si, trajectory=tr)
        replay = run(c.with_branches(m.branches), builder, seed=999, state_index=77, trajectory=3)  # forced: the names do not matter
        for other in (again, replay):
            assert other.logw == m.logw and np.array_equal(other.branches, m.branches)
            assert all(np.array_equal(a, b) for a, b in zip(other.tensors, m.tensors))


def test_draws_come_from_philox_stream_2(built):
    from qml_cutensornet_amd import engine

    seed = (0xDEADBEEF << 32) | 0x12345678
    for gate, traj, state in ((0, 0, 0), (7, 3, 2), (2 ** 32 - 1, 5, 9)):
        x = engine.philox4x32(np.array([gate, traj, state, 2], dtype=np.uint64), np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)).astype(np.uint64)
        u = float((int(x[0]) >> 5) * (1 << 26) + (int(x[1]) >> 6)) * 2.0 ** -53
        assert float(engine.channel_uniform(seed, gate, traj, state)) == u and 0.0 <= u < 1.0
    assert float(engine.channel_uniform(seed, 1, 2, 3)) != float(engine.sample_uniform(seed, 3, 2, 1))  # stream 0 is the sampler's
    # H then Measure on every qubit: p_0 = p_1 = 1/2 to rounding, so the branch is u >= 1/2 of the gate's own counter
    n, first = 6, 40
    gates = [g for q in range(n) for g in (("H", [q], []), ("Measure", [q], []))]
    c = from_gates(n, gates)
    at = np.flatnonzero(c.op == 10)
    for builder in BUILDERS:
        m, margin = run(c, builder, seed=seed, state_index=4, trajectory=6, first_gate=first, margin=True)
        u = engine.channel_uniform(seed, first + at, 6, 4)
        assert margin > 1e-6 and abs(margin - np.abs(u - 0.5).min()) < 1e-12
        assert m.branches.tolist() == (u >= 0.5).astype(int).tolist()
        assert abs(m.logw - n * math.log(0.5)) < 1e-12
        # state_index and trajectory change the draws (six fair coins each: these three sequences differ at this seed)
        others = [run(c, builder, seed=seed, state_index=si, trajectory=tr, first_gate=first).branches.tolist() for si, tr in ((5, 6), (4, 7))]
        assert m.branches.tolist() != others[0] and m.branches.tolist() != others[1] and others[0] != others[1]


def test_numpy_and_native_builder_draw_the_same_branches(built):
    n, gates, c = _noisy_8()
    for si, tr in ((0, 0), (1, 0), (1, 1), (2, 3)):
        a, margin = run(c, "numpy", seed=11, state_index=si, trajectory=tr, margin=True)
        assert margin >= 1e-6  # the condition of the comparison: no draw sits at a threshold (another seed if it ever does)
        b, margin_b = run(c, "native", seed=11, state_index=si, trajectory=tr, margin=True)
        assert np.array_equal(a.branches, b.branches) and abs(a.logw - b.logw) < 1e-12 and abs(margin - margin_b) < 1e-9
        assert abs(abs(np.vdot(mps_vector(a), mps_vector(b))) ** 2 - 1) < 1e-10


def _ok_program():
    """n = 4, two channel gates (positions 2 and 4): a drawn Depolarizing and a forced PostSelect."""
    return from_gates(4, [("H", [0], []), ("CX", [0, 1], []), ("Depolarizing", [1], [0.3]), ("Ry", [2], [0.4]), ("PostSelect", [0], [0]), ("CX", [2, 3], [])])


def bad_channel_programs():
    """[(label, circuit, text the error must hold)]; entry 0 is the good program."""
    ok = _ok_program()
    R = dataclasses.replace

    def arr(a, i, v):
        a = np.array(a, copy=True)
        a[i] = v
        return a

    off = ok.kraus.copy()
    off[0, 1] *= 1 + 2e-9
    forced_only = R(ok, kraus=off, branch=arr(ok.branch, 2, 1))
    return [
        ("ok", ok, ""),
        ("channel outside the table", R(ok, channel=arr(ok.channel, 2, 2)), "gate 2: channel index 2"),
        ("negative channel", R(ok, channel=arr(ok.channel, 4, -1)), "gate 4: channel index -1"),
        ("no Kraus matrix", R(ok, n_kraus=arr(ok.n_kraus, 0, 0)), "gate 2: .*Kraus matrices"),
        ("five Kraus matrices", R(ok, n_kraus=arr(ok.n_kraus, 1, 5)), "gate 4: .*Kraus matrices"),
        ("NaN", R(ok, kraus=arr(ok.kraus, (1, 1, 0, 1), np.nan)), "gate 4: .*not finite"),
        ("inf", R(ok, kraus=arr(ok.kraus, (0, 3, 1, 1), complex(0, np.inf))), "gate 2: .*not finite"),
        ("branch too large", R(ok, branch=arr(ok.branch, 2, 4)), "gate 2: branch 4"),
        ("branch below -1", R(ok, branch=arr(ok.branch, 4, -2)), "gate 4: branch -2"),
        ("drawn, not trace preserving by 4e-9", R(ok, kraus=off), "gate 2: .*not trace preserving"),
        ("drawn PostSelect projector", R(ok, kraus=arr(ok.kraus, (1, 1), 0.0), n_kraus=arr(ok.n_kraus, 1, 1), branch=arr(ok.branch, 4, -1)), "gate 4: .*not trace preserving"),
        ("outside the register", R(ok, q0=arr(ok.q0, 4, 4)), "gate 4.*outside the register"),
        ("code 10 without a table", R(ok, channel=None, branch=None, kraus=None, n_kraus=None), "unknown gate op code 10"),
        ("accepted: the same table with the branch forced", forced_only, None),
    ]


N_BAD_CHANNELS = 12


@pytest.mark.parametrize("builder", BUILDERS)
def test_rejections_name_the_gate(built, builder):
    progs = bad_channel_programs()
    assert len(progs) == N_BAD_CHANNELS + 2
    assert run(progs[0][1], builder).branches.shape == (2,)
    for label, c, text in progs[1:-1]:
        with pytest.raises(ValueError, match=text):
            run(c, builder)
    forced = run(progs[-1][1], builder)  # a forced branch may be any finite matrix
    assert forced.branches.tolist() == [1, 0]
    from qml_cutensornet_amd.ansatz import BoundCircuit

    for gate in (("AmplitudeDamping", [0], [1.5]), ("Kraus1q", [0], [[np.eye(2), np.eye(2)]]), ("PostSelect", [0], [2]), ("Measure", [0], [0.1]), ("Depolarizing", [4], [0.1]),
                 ("Kraus1q", [0], [[np.eye(2)] * 5]), ("Project", [0], [np.eye(3)])):
        with pytest.raises(ValueError):
            BoundCircuit.from_gates(4, [gate])
    for kw in ({"seed": -1}, {"state_index": 2 ** 32}, {"trajectory": -1}, {"first_gate": 0.5}):
        with pytest.raises(ValueError):
            run(progs[0][1], builder, **kw)


@pytest.mark.parametrize("builder", BUILDERS)
def test_an_impossible_postselection_names_state_and_gate(built, builder):
    c = from_gates(3, [("H", [0], []), ("X", [2], []), ("CX", [0, 1], []), ("PostSelect", [2], [0])])
    with pytest.raises(ValueError, match="state 7, gate 23"):
        run(c, builder, state_index=7, first_gate=20)
    assert run(from_gates(3, [("X", [2], []), ("PostSelect", [2], [1])]), builder).logw == 0.0


@pytest.mark.parametrize("builder", BUILDERS)
def test_a_program_without_channels_is_bit_equal_through_the_new_entry(built, builder):
    n = 8
    c = from_gates(n, brickwork(n, 4, features(1, n, 3)[0], seed=5, extras=[("CX", [6, 2], [])]))
    old = run(c, builder)
    table = _ok_program()
    none = np.full(c.op.shape, -1, dtype=np.int32)
    new = run(dataclasses.replace(c, channel=none, branch=none, kraus=table.kraus, n_kraus=table.n_kraus), builder, seed=5, state_index=3, trajectory=2, first_gate=9)
    assert new.fidelity == old.fidelity and new.logw == 0.0 and new.branches.shape == (0,) and old.logw == 0.0
    assert all(np.array_equal(a, b) for a, b in zip(new.tensors, old.tensors))


def test_gate_lists_templates_and_with_noise(built):
    import qml_cutensornet_amd as Q
    from qml_cutensornet_amd import ansatz as A
    from qml_cutensornet_amd.engine import with_noise

    assert A.OP_K1 == 10
    for name, params in (("AmplitudeDamping", [0.3]), ("PhaseDamping", [0.4]), ("Depolarizing", [0.2]), ("BitFlip", [0.1]), ("PhaseFlip", [0.25]), ("Measure", [])):
        K, branch = A.channel_kraus(name, params)
        assert branch == -1 and np.abs(K - np.array(kraus_of(name, params))).max() < 1e-16, name
    assert A.channel_kraus("PostSelect", [1])[1] == 1 and A.channel_kraus("Project", [np.eye(2)])[1] == 0
    gates = [("H", [0], []), ("XXPhase", [0, 2], [0.3]), ("Measure", [1], [])]
    noisy = with_noise(gates, "Depolarizing", [0.1])
    assert [g[0] for g in noisy] == ["H", "Depolarizing", "XXPhase", "Depolarizing", "Depolarizing", "Measure"] and [g[1] for g in noisy][3:5] == [[0], [2]]
    assert [g[0] for g in with_noise(gates, "BitFlip", [0.1], after="two_qubit")] == ["H", "XXPhase", "BitFlip", "BitFlip", "Measure"]
    with pytest.raises(ValueError):
        with_noise(gates, "Depolarizing", [0.1], after="some")
    c = from_gates(3, noisy)
    assert c.channel[c.op == 10].tolist() == [0, 1, 2, 3] and c.kraus.shape == (4, 4, 2, 2) and c.n_kraus.tolist() == [4, 4, 4, 2]  # a slot per channel gate
    names = [t[0] for t in c.as_tuples()]
    assert names.count("Kraus1q") == 4 and np.abs(c.as_tuples()[1][2][0] - np.array(kraus_of("Depolarizing", [0.1]))).max() < 1e-16
    again = from_gates(3, c.as_tuples())  # the routed program, emitted and read back
    assert np.array_equal(again.op, c.op) and np.array_equal(again.kraus, c.kraus)
    tail = c.sliced(3, c.n_gates)
    assert tail.n_channel_gates == c.op[3:].tolist().count(10) and tail.kraus is c.kraus
    back = pickle.loads(pickle.dumps(c))
    assert np.array_equal(back.channel, c.channel) and np.array_equal(back.kraus, c.kraus)
    # a template: the channel's parameters stand in the place of the angle and are constants of the ansatz
    ans = Q.CircuitAnsatz(3, [("H", [0], None), ("Rz", [1], (1.0, (1, 0, 1))), ("XXPhase", [0, 2], 0.3), ("AmplitudeDamping", [2], [0.2]), ("PostSelect", [0], [1])])
    a, b = ans.circuit_for_data([0.1, 0.2, 0.3]), ans.circuit_for_data([0.5, 0.6, 0.7])
    assert a.n_channel_gates == 2 and a.kraus is b.kraus and np.array_equal(a.channel, b.channel) and a.branch[a.op == 10].tolist() == [-1, 1]
    m = Q.simulate(a, seed=3, state_index=1)
    assert m.branches.shape == (2,) and m.branches[1] == 1 and m.logw < 0


def test_as_tuples_keeps_forced_branches_as_project(built):
    """A forced gate (PostSelect, Project with a matrix that preserves no trace, a replayed draw) comes out of ``as_tuples`` as
    ``Project`` with the forced matrix: read back, the program gives the same state and log-weight, bit for bit."""
    import qml_cutensornet_amd as Q

    M = np.array([[0.9, 0.2j], [0.0, 0.5]])
    c = from_gates(3, [("H", [0], []), ("CX", [0, 1], []), ("CX", [1, 2], []), ("AmplitudeDamping", [1], [0.3]), ("Project", [2], [M]), ("PostSelect", [0], [1])])
    first = Q.simulate(c, seed=4)
    forced = c.with_branches(first.branches)  # the drawn damping gate replayed
    tuples = forced.as_tuples()
    assert [t[0] for t in tuples if t[0] in ("Kraus1q", "Project")] == ["Project"] * 3 and [t[0] for t in c.as_tuples()].count("Kraus1q") == 1
    assert np.array_equal(tuples[-2][2][0], M) and np.array_equal(tuples[-1][2][0], np.diag([0.0, 1.0]))
    again = from_gates(3, tuples)
    assert again.branch[again.op == 10].tolist() == [0, 0, 0] and again.n_kraus.tolist() == [1, 1, 1]
    a, b = Q.simulate(forced), Q.simulate(again)
    assert a.logw == first.logw == b.logw and all(np.array_equal(x, y) for x, y in zip(a.tensors, b.tensors))


def test_paths_without_trajectories_reject_drawn_channels(built):
    """``simulate_many`` and ``builder_pool.build_states`` take no seed, state indices or trajectories (every state would draw as
    state 0, trajectory 0): a drawn channel is refused there; forced branches draw nothing and pass."""
    import qml_cutensornet_amd as Q
    from qml_cutensornet_amd import mps
    from qml_cutensornet_amd.builder_pool import build_states

    drawn = [("H", [0], None), ("XXPhase", [0, 1], 0.3), ("AmplitudeDamping", [1], [0.2])]
    forced = [("H", [0], None), ("XXPhase", [0, 1], 0.3), ("PostSelect", [1], [0])]
    X = np.array([[0.1, 0.2], [0.3, 0.4]])
    ans = Q.CircuitAnsatz(2, drawn)
    with pytest.raises(ValueError, match="drawn Kraus channels"):
        mps.simulate_many([ans.circuit_for_data(x) for x in X], workers=1)
    with pytest.raises(ValueError, match="drawn Kraus channels"):
        build_states(ans, X, 1 - 1e-16, workers=1)
    ok = Q.CircuitAnsatz(2, forced)
    states, _ = mps.simulate_many([ok.circuit_for_data(x) for x in X], workers=1)
    assert all(m.branches.tolist() == [0] and m.logw < 0 for m in states)


@pytest.mark.parametrize("builder", BUILDERS)
def test_capped_build_with_channels(built, builder):
    n, gates, c = _noisy_8()
    m = run(c, builder, max_bond=4, seed=11)
    assert m.max_bond() <= 4 and m.fidelity < 1 - 1e-3 and m.branches.min() >= 0 and np.isfinite(m.logw)
    v = mps_vector(m)
    assert abs(np.vdot(v, v).real - 1) < 1e-10
