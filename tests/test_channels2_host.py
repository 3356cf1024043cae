"""Two-qubit Kraus channels on the host (no GPU): op code 11 through both host builders against a dense density matrix and dense
state-vector trajectories written out here, the named two-qubit channels, forced branches and replay, the draws (Philox stream 2,
the counter of code 10), the agreement of the two builders' draws (behind a margin), identities with the matrix gates and with pairs
of one-qubit channels, routing, mixed programs, resume, a capped build, the rejections, and programs without code 11 through the new
entry.  The dense simulators, the circuits and the list of bad programs of this file are shared with tests/test_gpu_channels2.py."""
import dataclasses
import math

import numpy as np
import pytest

from test_channels_host import BUILDERS, CHANNELS, kraus_of, run
from test_matrix_gates_host import PREP, apply_dense, brickwork, dense_state, features, from_gates, gate_matrix, haar, mps_vector

CHANNELS2 = ("Kraus2q", "Project2q", "Depolarizing2q", "CorrelatedPhaseFlip", "Measure2q", "PostSelect2q")
_PAULI = [np.eye(2, dtype=complex), np.array([[0, 1], [1, 0]], dtype=complex), np.array([[0, -1j], [1j, 0]]), np.array([[1, 0], [0, -1]], dtype=complex)]


def kraus2_of(name, params):
    """The Kraus matrices of a named two-qubit channel (index (s_a, s_b), the first qubit most significant), written out here: the
    reference of this file, independent of the table under test."""
    if name in ("Kraus2q", "Project2q"):
        k = np.asarray(params[0], dtype=complex)
        return list(k) if k.ndim == 3 else [k]
    if name in ("Measure2q", "PostSelect2q"):
        return [np.diag(np.eye(4)[b]).astype(complex) for b in range(4)]
    p = float(params[0])
    if name == "CorrelatedPhaseFlip":
        return [math.sqrt(1 - p) * np.eye(4, dtype=complex), math.sqrt(p) * np.kron(_PAULI[3], _PAULI[3])]
    assert name == "Depolarizing2q"
    out = [math.sqrt(p / 16) * np.kron(P, Q) for P in _PAULI for Q in _PAULI]  # P-major over I, X, Y, Z
    out[0] = math.sqrt(1 - 15 * p / 16) * np.eye(4, dtype=complex)
    return out


def _matrices(name, params):
    if name in CHANNELS2:
        return kraus2_of(name, params), True
    if name in CHANNELS:
        return kraus_of(name, params), True
    return [gate_matrix(name, params[0] if params is not None and len(params) else None)], False


def dense_rho2(n, gates):
    """The density matrix of an unrouted gate list with the channels of either arity applied as Kraus maps, (2^n, 2^n)."""
    d = 2 ** n
    rho = np.zeros((d, d), dtype=complex)
    rho[0, 0] = 1.0

    def left(r, m, qubits):  # m on the row index of r
        return apply_dense(r.reshape((2,) * n + (d,)), m, qubits).reshape(d, d)

    for name, qubits, params in gates:
        ms, _ = _matrices(name, params)
        rho = sum(left(left(rho, m, list(qubits)).conj().T, m, list(qubits)).conj().T for m in ms)
    return rho


def dense_trajectory2(n, gates, branches):
    """The state vector of one trajectory: channel gate j (either arity) applies its Kraus matrix ``branches[j]`` and renormalises.
    Returns (psi, logw) with logw the sum of the logs of the branch probabilities."""
    psi = np.zeros((2,) * n, dtype=complex)
    psi[(0,) * n] = 1.0
    logw, j = 0.0, 0
    for name, qubits, params in gates:
        ms, is_channel = _matrices(name, params)
        if is_channel:
            psi = apply_dense(psi, ms[int(branches[j])], list(qubits))
            p = float(np.vdot(psi, psi).real)
            psi = psi / math.sqrt(p)
            logw += math.log(p)
            j += 1
        else:
            psi = apply_dense(psi, ms[0], list(qubits))
    assert j == len(branches)
    return psi.reshape(-1), logw


# n = 6: the entangling circuit of tests/test_channels_host.py with a Depolarizing2q(0.3) on the interior pair (1, 2) while the
# orthogonality centre sits on (4, 5), and a CorrelatedPhaseFlip(0.2) on the last pair: 16 x 2 forced-branch runs
ENUM2_GATES = [("H", [0], []), ("CX", [0, 1], []), ("Ry", [2], [0.3]), ("CX", [1, 2], []), ("XXPhase", [2, 3], [0.4]), ("CX", [3, 4], []), ("ZZPhase", [4, 5], [0.3]),
               ("Rx", [5], [0.7]), ("XXPhase", [4, 5], [0.6]), ("Depolarizing2q", [1, 2], [0.3]), ("CX", [2, 3], []), ("Ry", [5], [0.4]),
               ("CorrelatedPhaseFlip", [4, 5], [0.2]), ("YYPhase", [0, 1], [0.2])]
ENUM2_BRANCHES = [(b0, b1) for b0 in range(16) for b1 in range(2)]


def noisy2_brickwork(n, layers, x, seed, p=0.05):
    """The Haar brickwork of tests/test_matrix_gates_host.py with Depolarizing2q(p) behind every two-qubit gate (on the pair as the
    gate names it: every third one reversed) and a Measure2q in mid-chain after the first half of it."""
    from qml_cutensornet_amd.engine import with_noise

    gates = with_noise(brickwork(n, layers, x, seed=seed), "Depolarizing2q", [p], after="two_qubit")
    half = len(gates) // 2
    return gates[:half] + [("Measure2q", [n // 2 - 1, n // 2], [])] + gates[half:]


def _noisy2_8(seed_x=3):
    n = 8
    gates = noisy2_brickwork(n, 4, features(1, n, seed_x)[0], seed=5)
    return n, gates, from_gates(n, gates)


@pytest.mark.parametrize("builder", BUILDERS)
def test_exact_enumeration_of_two_two_qubit_channels(built, builder):
    n = 6
    c = from_gates(n, ENUM2_GATES)
    assert c.op.tolist().count(11) == 2 and c.n_channel_gates == 2 and c.q0[c.op == 11].tolist() == [1, 4] and c.n_kraus2.tolist() == [16, 2]
    want = dense_rho2(n, ENUM2_GATES)
    assert abs(np.trace(want).real - 1) < 1e-13
    rho, total = np.zeros_like(want), 0.0
    for b0, b1 in ENUM2_BRANCHES:
        m = run(c.with_branches([b0, b1]), builder)
        assert m.branches.tolist() == [b0, b1] and abs(m.fidelity - 1) < 1e-12
        v = mps_vector(m)
        assert abs(np.vdot(v, v).real - 1) < 1e-12  # back at norm 1
        rho += math.exp(m.logw) * np.outer(v, v.conj())
        total += math.exp(m.logw)
    assert abs(total - 1) < 1e-12
    assert np.abs(rho - want).max() < 1e-12


@pytest.mark.parametrize("builder", BUILDERS)
def test_drawn_trajectories_match_dense_trajectories_and_replay(built, builder):
    n, gates, c = _noisy2_8()
    assert c.n_channel_gates == sum(g[0] == "Unitary2q" for g in gates) + 1 and set(c.n_kraus2.tolist()) == {16, 4}
    for si, tr in ((0, 0), (0, 1), (5, 0)):
        m = run(c, builder, seed=11, state_index=si, trajectory=tr)
        assert m.branches.shape == (c.n_channel_gates,) and m.branches.min() >= 0
        psi, logw = dense_trajectory2(n, gates, m.branches)
        assert abs(abs(np.vdot(psi, mps_vector(m))) ** 2 - 1) < 1e-10
        assert abs(m.logw - logw) < 1e-12
        again = run(c, builder, seed=11, state_index=si, trajectory=tr)
        replay = run(c.with_branches(m.branches), builder, seed=999, state_index=77, trajectory=3)  # forced: the names do not matter
        for other in (again, replay):
            assert other.logw == m.logw and np.array_equal(other.branches, m.branches)
            assert all(np.array_equal(a, b) for a, b in zip(other.tensors, m.tensors))


def test_draws_come_from_philox_stream_2(built):
    """H (x) H then Measure2q on every pair: the four outcomes have probability 1/4 to rounding, so the branch is floor(4 u) of the
    gate's own counter (first_gate + i, trajectory, state_index, 2)."""
    from qml_cutensornet_amd import engine

    seed = (0xDEADBEEF << 32) | 0x12345678
    n, first = 6, 40
    gates = [g for q in range(0, n, 2) for g in (("H", [q], []), ("H", [q + 1], []), ("Measure2q", [q, q + 1], []))]
    c = from_gates(n, gates)
    at = np.flatnonzero(c.op == 11)
    u = engine.channel_uniform(seed, first + at, 6, 4)
    for builder in BUILDERS:
        m, margin = run(c, builder, seed=seed, state_index=4, trajectory=6, first_gate=first, margin=True)
        assert margin > 1e-6 and abs(margin - np.abs(u[:, None] - np.array([0.25, 0.5, 0.75])[None, :]).min()) < 1e-12
        assert m.branches.tolist() == np.floor(4 * u).astype(int).tolist()
        assert abs(m.logw - 3 * math.log(0.25)) < 1e-12
        others = [run(c, builder, seed=seed, state_index=si, trajectory=tr, first_gate=first).branches.tolist() for si, tr in ((5, 6), (4, 7))]
        assert m.branches.tolist() != others[0] and m.branches.tolist() != others[1] and others[0] != others[1]


def test_numpy_and_native_builder_draw_the_same_branches(built):
    n, gates, c = _noisy2_8()
    for si, tr in ((0, 0), (1, 0), (1, 1), (2, 3)):
        a, margin = run(c, "numpy", seed=11, state_index=si, trajectory=tr, margin=True)
        assert margin >= 1e-6  # the condition of the comparison: no draw sits at a threshold (another seed if it ever does)
        b, margin_b = run(c, "native", seed=11, state_index=si, trajectory=tr, margin=True)
        assert np.array_equal(a.branches, b.branches) and abs(a.logw - b.logw) < 1e-12 and abs(margin - margin_b) < 1e-9
        assert abs(abs(np.vdot(mps_vector(a), mps_vector(b))) ** 2 - 1) < 1e-10


@pytest.mark.parametrize("builder", BUILDERS)
def test_identities_with_unitaries_and_one_qubit_channels(built, builder):
    rng = np.random.default_rng(7)
    n = 4
    head = [("H", [0], []), ("CX", [0, 1], []), ("Ry", [2], [0.3]), ("CX", [1, 2], []), ("XXPhase", [2, 3], [0.4])]
    u = haar(rng, 4)
    want = run(from_gates(n, head + [("Unitary2q", [1, 2], [u]), ("CX", [2, 3], [])]), builder)
    # Depolarizing2q(0) (drawn: the only branch with weight is the identity) and Kraus2q of one unitary are the Unitary2q state
    for gates in (head + [("Unitary2q", [1, 2], [u]), ("Depolarizing2q", [1, 2], [0.0]), ("CX", [2, 3], [])], head + [("Kraus2q", [1, 2], [[u]]), ("CX", [2, 3], [])]):
        m = run(from_gates(n, gates), builder, seed=3)
        assert m.branches.tolist() == [0] and abs(m.logw) < 1e-13 and np.abs(mps_vector(m) - mps_vector(want)).max() < 1e-13
    # product matrices K (x) K' with forced branches: the state and the summed logw of two forced Kraus1q gates
    K, Kp = kraus_of("AmplitudeDamping", [0.3]), kraus_of("Depolarizing", [0.4])
    prod = [np.kron(a, b) for a in K for b in Kp]
    pair = from_gates(n, head + [("Kraus2q", [1, 2], [prod]), ("CX", [2, 3], [])])
    ones = from_gates(n, head + [("Kraus1q", [1], [K]), ("Kraus1q", [2], [Kp]), ("CX", [2, 3], [])])
    for ka in range(2):
        for kb in range(4):
            a, b = run(pair.with_branches([ka * 4 + kb]), builder), run(ones.with_branches([ka, kb]), builder)
            assert abs(a.logw - b.logw) < 1e-13 and np.abs(mps_vector(a) - mps_vector(b)).max() < 1e-13
    # PostSelect2q on a Bell pair inside a chain: the bond of the pair shrinks to 1
    bell = [("H", [1], []), ("CX", [1, 2], []), ("Ry", [0], [0.4]), ("Ry", [3], [0.3])]
    assert run(from_gates(n, bell), builder).tensors[1].shape[2] == 2
    for bits in (0, 3):
        m = run(from_gates(n, bell + [("PostSelect2q", [1, 2], [bits])]), builder)
        assert m.tensors[1].shape[2] == 1 and abs(m.logw - math.log(0.5)) < 1e-14 and m.branches.tolist() == [bits] and abs(m.fidelity - 1) < 1e-14
        psi, _ = dense_trajectory2(n, bell + [("PostSelect2q", [1, 2], [bits])], [bits])
        assert np.abs(mps_vector(m) - psi).max() < 1e-14
    # Measure2q on |00> + |11> never draws 01 or 10
    c = from_gates(n, bell + [("Measure2q", [1, 2], [])])
    drawn = {int(run(c, builder, seed=5, state_index=s).branches[0]) for s in range(24)}
    assert drawn == {0, 3}


@pytest.mark.parametrize("builder", BUILDERS)
def test_reversed_and_non_adjacent_pairs(built, builder):
    from qml_cutensornet_amd.ansatz import exchange_qubits

    rng = np.random.default_rng(9)
    n = 5
    head = PREP + [("CX", [1, 2], []), ("Ry", [3], [0.7]), ("CX", [2, 3], []), ("XXPhase", [3, 4], [0.3])]
    Ks = [0.8 * haar(rng, 4), 0.6 * haar(rng, 4)]  # sum K^H K = 1: trace preserving, not symmetric in the two qubits
    for b in (0, 1):
        # on [2, 1] every Kraus matrix acts with the qubit roles exchanged
        rev = run(from_gates(n, head + [("Kraus2q", [2, 1], [Ks])]).with_branches([b]), builder)
        fwd = run(from_gates(n, head + [("Kraus2q", [1, 2], [[exchange_qubits(k) for k in Ks]])]).with_branches([b]), builder)
        psi, logw = dense_trajectory2(n, head + [("Kraus2q", [2, 1], [Ks])], [b])
        assert rev.logw == fwd.logw and all(np.array_equal(x, y) for x, y in zip(rev.tensors, fwd.tensors))
        assert np.abs(mps_vector(rev) - psi).max() < 1e-13 and abs(rev.logw - logw) < 1e-13
        # a non-adjacent pair is the hand-routed SWAP chain
        far = from_gates(n, head + [("Kraus2q", [0, 3], [Ks])])
        hand = from_gates(n, head + [("SWAP", [0, 1], []), ("SWAP", [1, 2], []), ("Kraus2q", [2, 3], [Ks]), ("SWAP", [1, 2], []), ("SWAP", [0, 1], [])])
        assert np.array_equal(far.op, hand.op) and np.array_equal(far.q0, hand.q0) and far.op.tolist()[-5:] == [3, 3, 11, 3, 3]
        a, h = run(far.with_branches([b]), builder), run(hand.with_branches([b]), builder)
        psi, logw = dense_trajectory2(n, head + [("Kraus2q", [0, 3], [Ks])], [b])
        assert all(np.array_equal(x, y) for x, y in zip(a.tensors, h.tensors)) and np.abs(mps_vector(a) - psi).max() < 1e-13 and abs(a.logw - logw) < 1e-13


def mixed_gates():
    """n = 5, codes 10 and 11 interleaved: channel gates at program positions known to the tests."""
    return [("H", [0], []), ("CX", [0, 1], []), ("AmplitudeDamping", [1], [0.3]), ("CX", [1, 2], []), ("Depolarizing2q", [1, 2], [0.2]), ("Ry", [3], [0.4]), ("CX", [2, 3], []),
            ("Measure", [2], []), ("XXPhase", [3, 4], [0.3]), ("CorrelatedPhaseFlip", [4, 3], [0.25]), ("Depolarizing", [0], [0.2]), ("Measure2q", [0, 1], [])]


@pytest.mark.parametrize("builder", BUILDERS)
def test_mixed_programs_number_their_branches_in_program_order(built, builder):
    n, gates = 5, mixed_gates()
    c = from_gates(n, gates)
    assert c.op[np.isin(c.op, (10, 11))].tolist() == [10, 11, 10, 11, 10, 11] and c.n_channel_gates == 6
    assert c.channel[c.op == 10].tolist() == [0, 1, 2] and c.channel[c.op == 11].tolist() == [0, 1, 2]  # a slot per gate in each table
    seen = set()
    for si in range(6):
        m = run(c, builder, seed=21, state_index=si)
        limits = [2, 16, 2, 2, 4, 4]
        assert m.branches.shape == (6,) and all(0 <= b < k for b, k in zip(m.branches.tolist(), limits))
        psi, logw = dense_trajectory2(n, gates, m.branches)
        assert abs(abs(np.vdot(psi, mps_vector(m))) ** 2 - 1) < 1e-10 and abs(m.logw - logw) < 1e-12
        replay = run(c.with_branches(m.branches), builder)
        assert replay.logw == m.logw and all(np.array_equal(a, b) for a, b in zip(replay.tensors, m.tensors))
        seen.add(tuple(m.branches.tolist()))
    assert len(seen) > 1
    names = [t[0] for t in c.as_tuples()]
    assert names.count("Kraus2q") == 3 and names.count("Kraus1q") == 3
    rec = m.branches.tolist()  # a possible outcome: the last trajectory's
    forced = c.with_branches(rec[:5] + [-1]).as_tuples()
    assert [t[0] for t in forced if t[0].startswith(("Kraus", "Project"))] == ["Project", "Project2q", "Project", "Project2q", "Project", "Kraus2q"]
    assert np.abs(forced[4][2][0] - kraus2_of("Depolarizing2q", [0.2])[rec[1]]).max() < 1e-16
    again = from_gates(n, forced)  # the routed program, emitted and read back: the same state and logw
    a, b = run(c.with_branches(rec), builder), run(again.with_branches([0, 0, 0, 0, 0, rec[5]]), builder)
    assert a.logw == b.logw and all(np.array_equal(x, y) for x, y in zip(a.tensors, b.tensors))


def test_a_resumed_build_draws_what_the_uninterrupted_one_draws(built):
    """The numpy loop keeps snapshots: the tail of the program run with ``first_gate`` draws the uninterrupted run's branches (the
    native builder has no resume: it is given the same ``first_gate`` on a program whose head has no channel)."""
    from qml_cutensornet_amd import mps

    n, gates, c = _noisy2_8()
    cut = int(np.flatnonzero(c.op == 11)[3]) + 1
    whole = run(c, "numpy", seed=11, state_index=2, trajectory=1)
    snaps = mps._simulate(c, 1.0, 1e-16, None, [cut, c.n_gates], seed=11, state_index=2, trajectory=1)
    assert snaps[0].branches.tolist() == whole.branches[:4].tolist() and np.array_equal(snaps[1].branches, whole.branches) and snaps[1].logw == whole.logw
    # the uniform of gate i is that of position first_gate + i: a program shifted by `first_gate` draws from the shifted counters
    from qml_cutensornet_amd import engine

    two = from_gates(4, [("H", [1], []), ("H", [2], []), ("Measure2q", [1, 2], [])])
    for builder in BUILDERS:
        for first in (0, 17):
            m = run(two, builder, seed=5, state_index=3, trajectory=2, first_gate=first)
            assert m.branches.tolist() == [int(4 * float(engine.channel_uniform(5, first + 2, 2, 3)))]


@pytest.mark.parametrize("builder", BUILDERS)
def test_capped_build_with_two_qubit_channels(built, builder):
    n, gates, c = _noisy2_8()
    m = run(c, builder, max_bond=4, seed=11)
    assert m.max_bond() <= 4 and m.fidelity < 1 - 1e-3 and m.branches.min() >= 0 and np.isfinite(m.logw)
    v = mps_vector(m)
    assert abs(np.vdot(v, v).real - 1) < 1e-10


def _ok2_program():
    """n = 4, three channel gates (positions 2, 4, 5): a drawn Depolarizing2q, a forced PostSelect2q (behind an Ry that keeps its
    outcome possible whatever was drawn), a drawn one-qubit Depolarizing."""
    return from_gates(4, [("H", [0], []), ("CX", [0, 1], []), ("Depolarizing2q", [1, 2], [0.3]), ("Ry", [0], [0.4]), ("PostSelect2q", [0, 1], [0]), ("Depolarizing", [3], [0.1]),
                          ("CX", [2, 3], [])])


def bad_channel2_programs():
    """[(label, circuit, text the error must hold)]; entry 0 is the good program, the last one is accepted too."""
    ok = _ok2_program()
    R = dataclasses.replace

    def arr(a, i, v):
        a = np.array(a, copy=True)
        a[i] = v
        return a

    off = ok.kraus2.copy()
    off[0, 1] *= 1 + 2e-9
    forced_only = R(ok, kraus2=off, branch=arr(ok.branch, 2, 7))
    return [
        ("ok", ok, ""),
        ("channel outside the table", R(ok, channel=arr(ok.channel, 2, 2)), "gate 2: .*channel index 2"),
        ("negative channel", R(ok, channel=arr(ok.channel, 4, -1)), "gate 4: .*channel index -1"),
        ("no Kraus matrix", R(ok, n_kraus2=arr(ok.n_kraus2, 0, 0)), "gate 2: .*Kraus matrices"),
        ("seventeen Kraus matrices", R(ok, n_kraus2=arr(ok.n_kraus2, 1, 17)), "gate 4: .*Kraus matrices"),
        ("NaN", R(ok, kraus2=arr(ok.kraus2, (1, 1, 0, 1), np.nan)), "gate 4: .*not finite"),
        ("inf", R(ok, kraus2=arr(ok.kraus2, (0, 15, 3, 3), complex(0, np.inf))), "gate 2: .*not finite"),
        ("branch too large", R(ok, branch=arr(ok.branch, 2, 16)), "gate 2: branch 16"),
        ("branch below -1", R(ok, branch=arr(ok.branch, 4, -2)), "gate 4: branch -2"),
        ("drawn, not trace preserving by 4e-9", R(ok, kraus2=off), "gate 2: .*not trace preserving"),
        ("drawn PostSelect2q projector", R(ok, kraus2=arr(ok.kraus2, (1, slice(1, 4)), 0.0), n_kraus2=arr(ok.n_kraus2, 1, 1), branch=arr(ok.branch, 4, -1)),
         "gate 4: .*not trace preserving"),
        ("pair outside the register", R(ok, q0=arr(ok.q0, 2, 3)), "gate 2.*outside the register"),
        ("code 11 without a two-qubit table", R(ok, kraus2=None, n_kraus2=None), "unknown gate op code 11"),
        ("accepted: the same table with the branch forced", forced_only, None),
    ]


N_BAD_CHANNELS2 = 12


@pytest.mark.parametrize("builder", BUILDERS)
def test_rejections_name_the_gate(built, builder):
    progs = bad_channel2_programs()
    assert len(progs) == N_BAD_CHANNELS2 + 2
    assert run(progs[0][1], builder).branches.shape == (3,)
    for label, c, text in progs[1:-1]:
        with pytest.raises(ValueError, match=text):
            run(c, builder)
    forced = run(progs[-1][1], builder, seed=1)  # a forced branch may be any finite matrix
    assert forced.branches.tolist()[:2] == [7, 0]
    from qml_cutensornet_amd.ansatz import BoundCircuit

    for gate in (("Depolarizing2q", [0, 1], [1.5]), ("Kraus2q", [0, 1], [[np.eye(4), np.eye(4)]]), ("PostSelect2q", [0, 1], [4]), ("Measure2q", [0, 1], [0.1]),
                 ("Depolarizing2q", [3, 4], [0.1]), ("Kraus2q", [0, 1], [[np.eye(4) / 17 ** 0.5] * 17]), ("Project2q", [0, 1], [np.eye(2)]), ("CorrelatedPhaseFlip", [1, 1], [0.1]),
                 ("Measure2q", [0], [])):
        with pytest.raises(ValueError):
            BoundCircuit.from_gates(4, [gate])


@pytest.mark.parametrize("builder", BUILDERS)
def test_an_impossible_joint_postselection_names_state_and_gate(built, builder):
    c = from_gates(3, [("H", [0], []), ("X", [2], []), ("CX", [0, 1], []), ("PostSelect2q", [1, 2], [2])])  # qubit 2 is |1>: (1, 0) cannot happen
    with pytest.raises(ValueError, match="state 7, gate 23"):
        run(c, builder, state_index=7, first_gate=20)
    assert abs(run(from_gates(3, [("X", [2], []), ("PostSelect2q", [1, 2], [1])]), builder).logw) == 0.0


def test_paths_without_trajectories_reject_drawn_two_qubit_channels(built):
    import qml_cutensornet_amd as Q
    from qml_cutensornet_amd import mps
    from qml_cutensornet_amd.builder_pool import build_states

    drawn = [("H", [0], None), ("XXPhase", [0, 1], 0.3), ("CorrelatedPhaseFlip", [0, 1], [0.2])]
    forced = [("H", [0], None), ("XXPhase", [0, 1], 0.3), ("PostSelect2q", [1, 0], [0])]
    X = np.array([[0.1, 0.2], [0.3, 0.4]])
    ans = Q.CircuitAnsatz(2, drawn)
    a, b = ans.circuit_for_data(X[0]), ans.circuit_for_data(X[1])
    assert a.n_channel_gates == 1 and a.kraus2 is b.kraus2 and a.kraus is None and a.branch[a.op == 11].tolist() == [-1]
    with pytest.raises(ValueError, match="drawn Kraus channels"):
        mps.simulate_many([a, b], workers=1)
    with pytest.raises(ValueError, match="drawn Kraus channels"):
        build_states(ans, X, 1 - 1e-16, workers=1)
    ok = Q.CircuitAnsatz(2, forced)
    states, _ = mps.simulate_many([ok.circuit_for_data(x) for x in X], workers=1)
    assert all(m.branches.tolist() == [0] and m.logw < 0 for m in states)


def test_names_tables_and_with_noise(built):
    from qml_cutensornet_amd import ansatz as A
    from qml_cutensornet_amd.engine import with_noise

    assert A.OP_K2 == 11 and A.is_two_qubit(11)
    for name, params in (("Depolarizing2q", [0.3]), ("CorrelatedPhaseFlip", [0.2]), ("Measure2q", [])):
        K, branch = A.channel_kraus2(name, params)
        assert branch == -1 and np.abs(K - np.array(kraus2_of(name, params))).max() < 1e-16, name
    assert A.channel_kraus2("PostSelect2q", [2])[1] == 2 and A.channel_kraus2("Project2q", [np.eye(4)])[1] == 0
    gates = [("H", [0], []), ("XXPhase", [2, 0], [0.3]), ("Measure", [1], []), ("CX", [1, 2], [])]
    noisy = with_noise(gates, "Depolarizing2q", [0.1], after="two_qubit")  # ONE channel on the gate's pair, as the gate names it
    assert [(g[0], g[1]) for g in noisy] == [("H", [0]), ("XXPhase", [2, 0]), ("Depolarizing2q", [2, 0]), ("Measure", [1]), ("CX", [1, 2]), ("Depolarizing2q", [1, 2])]
    assert [g[0] for g in with_noise(gates, "BitFlip", [0.1], after="two_qubit")] == ["H", "XXPhase", "BitFlip", "BitFlip", "Measure", "CX", "BitFlip", "BitFlip"]
    with pytest.raises(ValueError, match="two_qubit"):
        with_noise(gates, "Depolarizing2q", [0.1], after="all")
    c = from_gates(3, noisy)
    assert c.channel[c.op == 11].tolist() == [0, 1] and c.kraus2.shape == (2, 16, 4, 4) and c.n_kraus2.tolist() == [16, 16] and c.kraus.shape == (1, 4, 2, 2)
    tail = c.sliced(3, c.n_gates)
    assert tail.kraus2 is c.kraus2 and tail.n_channel_gates == int(np.isin(c.op[3:], (10, 11)).sum())
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import _entangling_weight

    assert _entangling_weight(from_gates(3, [("CX", [0, 1], []), ("Depolarizing2q", [0, 1], [0.1])])) == 2.0


@pytest.mark.parametrize("builder", BUILDERS)
def test_programs_without_code_11_are_bit_equal_through_the_new_entry(built, builder):
    """A two-qubit table that no gate reads changes nothing: states, fidelities, logw and branches of a program without channels
    and of a program with code 10 are those of the old entry points, bit for bit."""
    from test_channels_host import _noisy_8

    table = _ok2_program()
    n = 8
    plain = from_gates(n, brickwork(n, 4, features(1, n, 3)[0], seed=5, extras=[("CX", [6, 2], [])]))
    none = np.full(plain.op.shape, -1, dtype=np.int32)
    _, _, noisy1 = _noisy_8()
    for old, new in ((plain, dataclasses.replace(plain, channel=none, branch=none, kraus2=table.kraus2, n_kraus2=table.n_kraus2)),
                     (noisy1, dataclasses.replace(noisy1, kraus2=table.kraus2, n_kraus2=table.n_kraus2))):
        a = run(old, builder, seed=11, state_index=3, trajectory=2, max_bond=6)
        b = run(new, builder, seed=11, state_index=3, trajectory=2, max_bond=6)
        assert a.fidelity == b.fidelity and a.logw == b.logw and np.array_equal(a.branches, b.branches)
        assert all(np.array_equal(x, y) for x, y in zip(a.tensors, b.tensors))
    assert run(noisy1, builder, seed=11, state_index=3, trajectory=2, max_bond=6).branches.shape == (noisy1.n_channel_gates,)
