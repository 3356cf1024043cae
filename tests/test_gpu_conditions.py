"""GPU tests of classical control in the device builder (``qk_build_mps_conditions``): teleportation and active reset read with
``local_paulis``; the 12-qubit, six-layer Haar brickwork of tests/test_conditions_host.py -- a Measure, a Measure2q and conditional
gates of every kind in mid-circuit -- against the host builder in the one-, two- and four-workgroup shapes; bit identity run to
run, of a state alone, in a set and in another order, and of the replay of the recorded branches (-2 included); a workgroup that
builds more than one state; checkpoints in front of, on and behind conditional gates and a resume; the rejections of the C entry;
the bits of a program without conditions against the build before this feature (tests/golden/conditions_parent_bits.json); and
the two noisy kernel drivers on a pooling ansatz.

Tolerances as tests/test_gpu_channels2.py: branches equal, |<dev|host>|^2 = 1 within 1e-10, log-weights within 1e-10, the capped
build |f_dev - f_host| < 1e-9 max(1, f_host), the drivers within 1e-9.  Device and host draw the same branches when no draw of the
host sits within 1e-6 of a threshold: asserted first (here and in tests/test_conditions_host.py), a condition of the comparison."""
import json
import math
import os

import numpy as np
import pytest

from oracle import restatement as R
from test_conditions_host import (N_BAD_CONDITIONS, RESET_GATES, SEED, STATE_INDEX, TRAJECTORY, bad_condition_programs, cond_12_circuits, runs_and_skips,
                                  teleport_gates, teleported_bloch)
from test_feature_map_host import zz_template
from test_gpu_channels import _bloch, same_bits
from test_gpu_channels2 import noisy2_12_gates, trajectory_digests
from test_matrix_gates_host import features, from_gates, haar, mps_vector

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(seed=SEED, state_index=STATE_INDEX, trajectory=TRAJECTORY)


def host_states(circuits, **kw):
    import qml_cutensornet_amd as Q

    host, margin = [], np.inf
    for c, s, t in zip(circuits, STATE_INDEX, TRAJECTORY):
        m, mg = Q.simulate(c, 1 - 1e-16, seed=SEED, state_index=int(s), trajectory=int(t), margin=True, **kw)
        host.append(m)
        margin = min(margin, mg)
    return host, margin


@pytest.fixture(scope="module")
def cond_12(built):
    """3 states x 2 trajectories: (circuits, host states, host margin)."""
    circuits = cond_12_circuits()
    return (circuits,) + host_states(circuits)


@pytest.fixture(scope="module")
def dev_12(gpu_ctx, cond_12):
    return gpu_ctx.build_mps(cond_12[0], **KW)


# ---- 1. teleportation and reset
def test_teleportation_and_reset_on_the_device(gpu_ctx):
    c = from_gates(3, teleport_gates())
    want = teleported_bloch()
    records = [[m0, m1] for m0 in (0, 1) for m1 in (0, 1)]
    xs, info = gpu_ctx.build_mps_set([c.with_branches(r) for r in records] + [c] * 8, seed=SEED, state_index=np.arange(12), trajectory=np.zeros(12, dtype=np.int64))
    with xs:
        bloch = np.asarray(gpu_ctx.local_paulis(xs))  # (n_states, n_qubits, 3)
    assert info["branches"][:4].tolist() == records and len({tuple(r) for r in info["branches"][4:].tolist()}) >= 2
    assert np.abs(bloch[:, 2, :] - want[None, :]).max() < 1e-12 and np.abs(info["logw"] - math.log(0.25)).max() < 1e-12
    bare, _ = gpu_ctx.build_mps_set([from_gates(3, teleport_gates(False)).with_branches(r) for r in records])
    with bare:
        off = np.abs(np.asarray(gpu_ctx.local_paulis(bare))[:, 2, :] - want[None, :]).max(axis=1)
    assert off[0] < 1e-12 and off[1:].min() > 0.05  # without the two conditional gates only outcome 00 teleports
    reset, info = gpu_ctx.build_mps_set([from_gates(1, RESET_GATES)] * 16, seed=SEED, state_index=np.arange(16))
    with reset:
        z = np.asarray(gpu_ctx.local_paulis(reset))[:, 0, 2]
    assert set(info["branches"][:, 0].tolist()) == {0, 1} and np.abs(z - 1).max() < 1e-14


# ---- 2. the 12-qubit program against the host builder
@pytest.mark.parametrize("wgs", ["1", "2"])
def test_device_builder_matches_host_builder_on_the_conditional_brickwork(gpu_ctx, cond_12, monkeypatch, wgs):
    monkeypatch.setenv("QK_BUILD_WGS", wgs)
    circuits, host, margin = cond_12
    c0 = circuits[0]
    assert sorted(set(c0.op[c0.cond_gate >= 0].tolist())) == [1, 2, 3, 6, 8, 9, 10, 11]
    assert margin >= 1e-6  # the condition of the comparison (asserted in tests/test_conditions_host.py too)
    dev, info = gpu_ctx.build_mps(circuits, **KW)
    print(f"classical control, n = 12, six Haar layers, {int(np.count_nonzero(c0.cond_gate >= 0))} conditional ops, 6 states, QK_BUILD_WGS={wgs}: kernel_ms = {info['kernel_ms']:.3f}")
    assert max(m.max_bond() for m in host) == 64  # the theta product of the widest gates runs on the matrix cores
    ran = np.array([runs_and_skips(c, m.branches) for c, m in zip(circuits, host)])
    assert ran.any(axis=0).all() and (~ran).any(axis=0).all()  # every conditional gate runs in one state and is skipped in another
    assert info["branches"].shape == (6, c0.n_channel_gates) and info["branches"].min() == -2
    for s, (md, mh) in enumerate(zip(dev, host)):
        assert np.array_equal(md.branches, mh.branches) and np.array_equal(info["branches"][s], mh.branches)
        assert np.array_equal(md.bond_dims(), mh.bond_dims())
        assert abs(abs(R.mps_inner(md.tensors, mh.tensors)) ** 2 - 1) < 1e-10
        assert abs(md.logw - mh.logw) < 1e-10 and info["logw"][s] == md.logw
        assert abs(md.fidelity - mh.fidelity) < 1e-9 * max(1.0, mh.fidelity)


def test_four_workgroup_shape_capped_at_bond_32(gpu_ctx, cond_12, monkeypatch):
    circuits = cond_12[0]
    monkeypatch.setenv("QK_BUILD_WGS", "1")
    cus = gpu_ctx.build_mps(circuits[:1], max_bond=32, truncate=True, seed=SEED, state_index=STATE_INDEX[:1], trajectory=TRAJECTORY[:1])[1]["slots"]  # one workgroup per CU
    monkeypatch.setenv("QK_BUILD_WGS", "4")
    host, margin = host_states(circuits, max_bond=32)
    assert margin >= 1e-6
    dev, info = gpu_ctx.build_mps(circuits, max_bond=32, truncate=True, **KW)
    print(f"classical control capped at 32, QK_BUILD_WGS=4: kernel_ms = {info['kernel_ms']:.3f}")
    assert not info["dropped"] and info["threads"] == 256 and info["slots"] == 4 * cus and info["grid"] == len(circuits)
    assert info["branches"].min() == -2 and max(h.max_bond() for h in host) == 32 and min(h.fidelity for h in host) < 1 - 1e-7  # skips; the cap cuts
    for d, h in zip(dev, host):
        print(f"capped at 32: device fidelity {d.fidelity:.15e}, host {h.fidelity:.15e}, difference {d.fidelity - h.fidelity:.3e}; logw {d.logw:.12f} / {h.logw:.12f}")
        assert np.array_equal(d.branches, h.branches)
        assert d.max_bond() <= 32 and abs(d.fidelity - h.fidelity) < 1e-9 * max(1.0, h.fidelity)
        assert np.array_equal(d.bond_dims(), h.bond_dims()) and abs(abs(R.mps_inner(d.tensors, h.tensors)) ** 2 - 1) < 1e-10 and abs(d.logw - h.logw) < 1e-10


# ---- 3. bit identity
def test_bit_identity_run_to_run_alone_in_a_set_and_replayed(gpu_ctx, cond_12, dev_12):
    circuits = cond_12[0]
    dev, _ = dev_12
    again, _ = gpu_ctx.build_mps(circuits, **KW)
    assert any(-2 in m.branches for m in dev)
    replay, _ = gpu_ctx.build_mps([c.with_branches(m.branches) for c, m in zip(circuits, dev)], seed=SEED + 1, state_index=STATE_INDEX[::-1].copy())
    for a, b, c in zip(dev, again, replay):
        assert same_bits(a, b) and same_bits(a, c)
    alone, _ = gpu_ctx.build_mps([circuits[3]], seed=SEED, state_index=int(STATE_INDEX[3]), trajectory=int(TRAJECTORY[3]))
    assert same_bits(alone[0], dev[3])
    order = [4, 1, 5]
    some, _ = gpu_ctx.build_mps([circuits[k] for k in order], seed=SEED, state_index=STATE_INDEX[order], trajectory=TRAJECTORY[order])
    for m, k in zip(some, order):
        assert same_bits(m, dev[k])


# ---- 4. a workgroup that builds more than one state
def turn_gates(x):
    """n = 8: two entangling layers, a Measure and a Measure2q, conditional gates of both arities and a conditional channel."""
    n = 8
    gates = [("H", [q], []) for q in range(n)] + [("ZZPhase", [q, q + 1], [float(x[q])]) for q in range(0, n - 1, 2)] + [("Ry", [q], [float(x[q])]) for q in range(n)]
    gates += [("XXPhase", [q, q + 1], [float(x[q + 1])]) for q in range(1, n - 1, 2)]
    A = len(gates)
    gates += [("Measure", [3], []), ("Measure2q", [5, 6], []), ("X", [2], [], (A, 1)), ("XXPhase", [3, 4], [0.3], (A + 1, [1, 2])), ("BitFlip", [4], [0.4], (A, 0)),
              ("CX", [0, 2], [], (A + 4, 1)), ("Rz", [7], [float(x[7])], (A + 1, [0, 3]))]
    return gates + [("YYPhase", [q, q + 1], [float(x[q]) * 0.5]) for q in range(0, n - 1, 2)]


def test_later_turn_states_are_the_bits_of_first_turn_states(gpu_ctx, monkeypatch):
    monkeypatch.setenv("QK_BUILD_WGS", "4")
    X = features(4, 8, 77)
    base = [from_gates(8, turn_gates(x)) for x in X]
    kw = dict(max_bond=16, seed=SEED)
    first, probe = gpu_ctx.build_mps(base, state_index=np.arange(4), **kw)
    slots = probe["slots"]
    assert probe["threads"] == 256 and probe["grid"] == 4 < slots
    n_states = slots + 8
    circuits = [base[k % 4] for k in range(n_states)]
    idx = np.arange(n_states)
    dev, info = gpu_ctx.build_mps(circuits, state_index=idx, **kw)
    print(f"turns: {n_states} states on a grid of {info['grid']} x {info['threads']} threads ({info['slots']} slots), kernel_ms = {info['kernel_ms']:.1f}")
    assert info["threads"] == 256 and info["grid"] == info["slots"] == slots < n_states
    assert info["branches"].min() == -2 and len({tuple(r) for r in info["branches"].tolist()}) > 8
    # every state again as the first of its workgroup: chunks of at most slots // 2 states
    size = slots // 2
    for s0 in range(0, n_states, size):
        part, pinfo = gpu_ctx.build_mps(circuits[s0:s0 + size], state_index=idx[s0:s0 + size], **kw)
        assert pinfo["grid"] == len(part) <= slots // 2
        for k, (a, b) in enumerate(zip(part, dev[s0:s0 + size])):
            assert same_bits(a, b), f"state {s0 + k}"
    for k in range(4):
        assert same_bits(first[k], dev[k])


# ---- 5. checkpoints and resume
def test_checkpoints_and_resume_around_conditional_gates(gpu_ctx, cond_12, dev_12):
    circuits = cond_12[0]
    dev, _ = dev_12
    c0 = c = circuits[0]
    at = np.flatnonzero(c0.cond_gate >= 0)
    chan = np.flatnonzero(np.isin(c0.op, (10, 11)))
    first_cond_channel = int(chan[np.isin(chan, at)][0])  # the conditional Depolarizing
    # in front of the first conditional gate, on a conditional gate (it is the next one), behind the conditional channels, the whole program
    cps = [int(at[0]), int(at[3]), first_cond_channel + 1, int(at[-1]) + 1, c0.n_gates]
    with gpu_ctx.build_mps_scan(circuits, cps, **KW) as scan:
        final = scan.states(-1)
        for a, b in zip(final, dev):  # the snapshots are copies: the run is the run without them
            assert same_bits(a, b)
        for j, cp in enumerate(cps[:-1]):
            snap, done = scan.states(j), int(np.count_nonzero(chan < cp))
            for m, f in zip(snap, final):
                assert np.array_equal(m.branches, f.branches[:done])
        # a resume whose remaining program keeps its conditions inside itself: from in front of the two measurements
        start = int(chan[0])
        assert start < at[0] and all(c.cond_gate[c.cond_gate >= 0].min() >= start for c in circuits)
    with gpu_ctx.build_mps_scan(circuits, [start, c0.n_gates], **KW) as scan:
        with gpu_ctx.build_mps_scan([c.sliced(start, c.n_gates) for c in circuits], [c0.n_gates - start], initial=(scan, 0), **KW) as resumed:
            assert resumed.first_gate == start
            for a, b in zip(resumed.states(-1), dev):
                assert a.fidelity == b.fidelity and a.logw == b.logw and np.array_equal(a.branches, b.branches)
                assert all(np.array_equal(x, y) for x, y in zip(a.tensors, b.tensors))
    with pytest.raises(ValueError, match="lies in front of the slice"):
        c.sliced(int(at[0]), c.n_gates)  # a slice that reaches behind the snapshot


# ---- 6. the C entry
@pytest.mark.parametrize("case", range(1, N_BAD_CONDITIONS + 1))
def test_device_entry_rejects_bad_condition_rows(gpu_ctx, case):
    from qml_cutensornet_amd.engine import QkError

    label, c, text = bad_condition_programs()[case]
    with pytest.raises(QkError, match=text):
        gpu_ctx.build_mps([c, c])


def test_device_entry_without_rows_is_the_two_qubit_channel_entry(gpu_ctx):
    from test_gpu_program_entry import BUILD_MPS, build_legacy, gate_program

    ok = bad_condition_programs()[0][1]
    dev, info = gpu_ctx.build_mps([ok] * 4, seed=3)
    assert info["branches"].shape == (4, 2) and all(abs(m.fidelity - 1) < 1e-12 for m in dev)
    circuits = [from_gates(12, noisy2_12_gates(x)) for x in features(2, 12, 41)]
    kw = dict(seed=SEED, state_index=np.array([0, 1]), trajectory=np.array([1, 0]))
    gp = gate_program(circuits, **kw)
    assert gp.cond_gate is None and gp.n_channels2 > 0
    with build_legacy(gpu_ctx, "qk_build_mps_channels2", gp, **BUILD_MPS) as scan:  # the C entries themselves, through ctypes
        old = scan.states(0)
    with build_legacy(gpu_ctx, "qk_build_mps_conditions", gp, **BUILD_MPS) as scan:  # cond_gate = NULL
        new = scan.states(0)
    assert all(same_bits(a, b) for a, b in zip(old, new))
    through_engine, _ = gpu_ctx.build_mps(circuits, **kw)
    assert all(same_bits(a, b) for a, b in zip(old, through_engine))
    none = np.full(circuits[0].op.shape, -1, dtype=np.int32)
    import dataclasses

    rows, _ = gpu_ctx.build_mps([dataclasses.replace(c, cond_gate=none, cond_mask=np.zeros(none.shape, dtype=np.uint32)) for c in circuits], **kw)  # rows that condition nothing
    assert all(same_bits(a, b) for a, b in zip(old, rows))


# ---- 7. the bits of the build before this feature
def parent_bits_program():
    """The ``noisy2_12`` build of tests/test_gpu_channels2.py: channel gates of code 11 behind every two-qubit gate, no conditions."""
    circuits = [from_gates(12, noisy2_12_gates(x)) for x in features(3, 12, 41) for _ in range(2)]
    return circuits, dict(seed=2024, state_index=np.array([0, 0, 1, 1, 2, 2]), trajectory=np.array([0, 1, 0, 1, 0, 1]))


def test_programs_without_conditions_download_the_bits_of_the_parent_build(gpu_ctx):
    """tests/golden/conditions_parent_bits.json was recorded once with ``trajectory_digests(gpu_ctx.build_mps(circuits, **kw)[0])``
    of ``parent_bits_program()`` from the commit before classical control was added."""
    circuits, kw = parent_bits_program()
    assert 11 in circuits[0].op and circuits[0].cond_gate is None
    with open(os.path.join(ROOT, "tests", "golden", "conditions_parent_bits.json")) as fp:
        want = json.load(fp)
    assert trajectory_digests(gpu_ctx.build_mps(circuits, **kw)[0]) == want["states"]


# ---- 8. the drivers
def pooling_ansatz(n=8):
    """A pooling layer: the ZZ feature map entangles, the odd qubits are measured, and each even neighbour is rotated by a Haar
    unitary where the outcome was 1."""
    import qml_cutensornet_amd as Q

    gates = list(zz_template(n, 2, 0.8, 2))
    A = len(gates)
    rng = np.random.default_rng(5)
    gates += [("Measure", [q], None) for q in range(1, n, 2)]
    gates += [("Unitary1q", [q - 1], haar(rng, 2), (A + k, 1)) for k, q in enumerate(range(1, n, 2))]
    return Q.CircuitAnsatz(n, gates)


@pytest.mark.parametrize("builder", ["device", "host"])
def test_noisy_kernel_drivers_on_a_pooling_ansatz(built, monkeypatch, builder):
    import qml_cutensornet_amd as Q
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_noisy_kernel_matrix, build_noisy_projected_kernel_matrix

    monkeypatch.setenv("QK_BUILDER", builder)
    n, T, seed = 8, 3, 8
    ans = pooling_ansatz(n)
    c = ans.circuit_for_data(np.zeros(n))
    assert c.n_channel_gates == 4 and int(np.count_nonzero(c.cond_gate >= 0)) == 4
    X = R.synthetic_features(4, n, 13)
    vx, margin, skipped = [], np.inf, 0
    for p, x in enumerate(X):
        row = []
        for t in range(T):
            m, mg = Q.simulate(ans.circuit_for_data(x), 1 - 1e-16, seed=seed, state_index=p, trajectory=t, margin=True)
            row.append(mps_vector(m))
            margin = min(margin, mg)
            skipped += int(np.count_nonzero(m.branches == 0))
        vx.append(row)
    assert margin >= 1e-6 and 0 < skipped < 4 * 4 * T  # conditional gates run and are skipped
    fx = np.array([np.mean([_bloch(v, n) for v in row], axis=0) for row in vx])
    K = build_noisy_projected_kernel_matrix(SingleComm(), ans, X, trajectories=T, noise_seed=seed, truncation_error=1e-16)
    want = np.exp(-0.5 / n * ((fx[:, None] - fx[None, :]) ** 2).sum(axis=(2, 3)))
    assert K.shape == (4, 4) and np.abs(K - want).max() < 1e-9
    F = build_noisy_kernel_matrix(SingleComm(), ans, X, trajectories=T, noise_seed=seed, truncation_error=1e-16)
    ref = np.zeros((4, 4))
    for j, rb in enumerate(vx):
        for i, ra in enumerate(vx):
            o = np.array([[abs(np.vdot(p, q)) ** 2 for p in ra] for q in rb])
            ref[j, i] = (o.sum() - np.trace(o)) / (T * (T - 1)) if i == j else o.mean()
    assert F.shape == (4, 4) and np.abs(F - ref).max() < 1e-9
