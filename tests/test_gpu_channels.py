"""GPU tests of the Kraus channels (op code 10) in the device builder: a noisy Haar brickwork against the host builder, the exact
enumeration of two damping gates against a dense density matrix, replay, independence of a state from its set, snapshots and resume,
a capped build, the rejections and the run-time error of ``qk_build_mps_channels``, the two noisy kernel drivers, and the bits of a
program without channels against the build before this op code existed (tests/golden/channels_parent_bits.json).

Tolerances as tests/test_gpu_matrix_gates.py: fidelity within 1e-12 of 1, |<dev|host>|^2 = 1 within 1e-10, the capped build
|f_dev - f_host| < 1e-9 max(1, f_host); log-weights within 1e-10, the dense density matrix within 1e-10, the drivers within 1e-9.
Device and host draw the same branches when no draw of the host sits within 1e-6 of a threshold: asserted first, a condition of the
comparison, not a measurement."""
import dataclasses
import hashlib
import json
import math
import os
import sys

import numpy as np
import pytest

from oracle import restatement as R
from test_channels_host import ENUM_GATES, N_BAD_CHANNELS, bad_channel_programs, dense_rho
from test_feature_map_host import zz_template
from test_matrix_gates_host import brickwork, features, from_gates, mps_vector
from test_projected_dist_host import pair_dist_from_dense
from test_projected_pair_host import ref_pair_gram

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = [("CX", [7, 6], []), ("CZ", [2, 5], [])]
SEED = 2024
STATE_INDEX = np.array([0, 0, 1, 1, 2, 2])
TRAJECTORY = np.array([0, 1, 0, 1, 0, 1])


def noisy_12_gates(x, measure=True):
    """n = 12: the six-layer Haar brickwork of tests/test_gpu_matrix_gates.py, AmplitudeDamping(0.05) behind every two-qubit gate on
    both of its qubits and a Measure in mid-chain after the third layer."""
    from qml_cutensornet_amd.engine import with_noise

    n = 12
    first, rest = brickwork(n, 3, x, seed=17), brickwork(n, 6, x, seed=17, extras=EXTRAS)
    assert len(rest) > len(first) and all(a[0] == b[0] and a[1] == b[1] and np.array_equal(np.asarray(a[2]), np.asarray(b[2])) for a, b in zip(first, rest))
    gates = rest[: len(first)] + ([("Measure", [6], [])] if measure else []) + rest[len(first):]
    return with_noise(gates, "AmplitudeDamping", [0.05], after="two_qubit")


@pytest.fixture(scope="module")
def noisy_12(built):
    """3 states x 2 trajectories: (circuits, host states, host margin)."""
    import qml_cutensornet_amd as Q

    circuits = [from_gates(12, noisy_12_gates(x)) for x in features(3, 12, 41) for _ in range(2)]
    host, margin = [], np.inf
    for c, s, t in zip(circuits, STATE_INDEX, TRAJECTORY):
        m, mg = Q.simulate(c, 1 - 1e-16, seed=SEED, state_index=int(s), trajectory=int(t), margin=True)
        host.append(m)
        margin = min(margin, mg)
    return circuits, host, margin


@pytest.fixture(scope="module")
def dev_12(gpu_ctx, noisy_12):
    circuits, _, _ = noisy_12
    return gpu_ctx.build_mps(circuits, seed=SEED, state_index=STATE_INDEX, trajectory=TRAJECTORY)


def same_bits(a, b):
    return a.fidelity == b.fidelity and a.logw == b.logw and np.array_equal(a.branches, b.branches) and len(a.tensors) == len(b.tensors) and all(
        np.array_equal(x, y) for x, y in zip(a.tensors, b.tensors))


@pytest.mark.parametrize("wgs", ["1", "2"])
def test_device_builder_matches_host_builder_on_a_noisy_brickwork(gpu_ctx, noisy_12, monkeypatch, wgs):
    monkeypatch.setenv("QK_BUILD_WGS", wgs)
    circuits, host, margin = noisy_12
    assert circuits[0].n_channel_gates == 2 * int(np.count_nonzero(circuits[0].op == 9)) + 1
    assert margin >= 1e-6  # the condition of the comparison (another SEED if it ever fails)
    dev, info = gpu_ctx.build_mps(circuits, seed=SEED, state_index=STATE_INDEX, trajectory=TRAJECTORY)
    print(f"channels, n = 12, six Haar layers, {circuits[0].n_channel_gates} channel gates, 6 states, QK_BUILD_WGS={wgs}: kernel_ms = {info['kernel_ms']:.3f}")
    assert max(m.max_bond() for m in host) >= 32
    assert info["branches"].shape == (6, circuits[0].n_channel_gates) and info["branches"].min() >= 0
    for s, (md, mh) in enumerate(zip(dev, host)):
        assert np.array_equal(md.branches, mh.branches) and np.array_equal(info["branches"][s], mh.branches)
        assert np.array_equal(md.bond_dims(), mh.bond_dims())
        assert abs(abs(R.mps_inner(md.tensors, mh.tensors)) ** 2 - 1) < 1e-10
        assert abs(md.logw - mh.logw) < 1e-10 and info["logw"][s] == md.logw
        assert abs(md.fidelity - 1.0) < 1e-12
    assert len({tuple(m.branches.tolist()) for m in dev}) > 1  # the trajectories differ


def test_damping_alone_keeps_bond_64_and_the_qr_centre_moves(gpu_ctx, monkeypatch):
    """The projective Measure halves the middle bond (32 at most in the circuits above).  Without it the bonds reach 64: centre moves
    of sites with 48 and more columns (Gram-Schmidt twice) run between the channel gates."""
    import qml_cutensornet_amd as Q

    monkeypatch.setenv("QK_BUILD_WGS", "2")
    c = from_gates(12, noisy_12_gates(features(3, 12, 41)[1], measure=False))
    host, margin = Q.simulate(c, 1 - 1e-16, seed=SEED, state_index=0, trajectory=0, margin=True)  # (a trajectory whose late gates do not decay)
    assert margin >= 1e-6 and host.max_bond() == 64
    dev, _ = gpu_ctx.build_mps([c], seed=SEED, state_index=0, trajectory=0)
    assert np.array_equal(dev[0].branches, host.branches) and np.array_equal(dev[0].bond_dims(), host.bond_dims())
    assert abs(abs(R.mps_inner(dev[0].tensors, host.tensors)) ** 2 - 1) < 1e-10 and abs(dev[0].logw - host.logw) < 1e-10 and abs(dev[0].fidelity - 1) < 1e-12


def test_exact_enumeration_on_the_device(gpu_ctx):
    """The n = 6 case of the host tests as four states of one call with per-state branch rows."""
    n = 6
    c = from_gates(n, ENUM_GATES)
    rows = [(b0, b1) for b0 in (0, 1) for b1 in (0, 1)]
    dev, info = gpu_ctx.build_mps([c.with_branches(r) for r in rows])
    assert info["branches"].tolist() == [list(r) for r in rows]
    rho, total = np.zeros((2 ** n, 2 ** n), dtype=complex), 0.0
    for m in dev:
        v = mps_vector(m)
        assert abs(np.vdot(v, v).real - 1) < 1e-12
        rho += math.exp(m.logw) * np.outer(v, v.conj())
        total += math.exp(m.logw)
    assert abs(total - 1) < 1e-10 and np.abs(rho - dense_rho(n, ENUM_GATES)).max() < 1e-10


def test_replay_and_run_to_run_are_bit_identical(gpu_ctx, noisy_12, dev_12):
    circuits, _, _ = noisy_12
    dev, _ = dev_12
    again, _ = gpu_ctx.build_mps(circuits, seed=SEED, state_index=STATE_INDEX, trajectory=TRAJECTORY)
    replay, _ = gpu_ctx.build_mps([c.with_branches(m.branches) for c, m in zip(circuits, dev)], seed=SEED + 1, state_index=STATE_INDEX[::-1].copy())
    for a, b, c in zip(dev, again, replay):
        assert same_bits(a, b) and same_bits(a, c)


def test_a_state_does_not_depend_on_its_set(gpu_ctx, noisy_12, dev_12):
    circuits, _, _ = noisy_12
    dev, _ = dev_12
    alone, _ = gpu_ctx.build_mps([circuits[3]], seed=SEED, state_index=int(STATE_INDEX[3]), trajectory=int(TRAJECTORY[3]))
    assert same_bits(alone[0], dev[3])
    order = [4, 1, 5]  # other states, another order
    some, _ = gpu_ctx.build_mps([circuits[k] for k in order], seed=SEED, state_index=STATE_INDEX[order], trajectory=TRAJECTORY[order])
    for m, k in zip(some, order):
        assert same_bits(m, dev[k])
    other, _ = gpu_ctx.build_mps([circuits[3]], seed=SEED, state_index=int(STATE_INDEX[3]), trajectory=7)
    assert not np.array_equal(other[0].branches, dev[3].branches)  # (66 draws: another trajectory is another sequence at this seed)


def test_snapshots_and_resume_with_first_gate(gpu_ctx, noisy_12, dev_12):
    circuits, _, _ = noisy_12
    dev, _ = dev_12
    c0 = circuits[0]
    at = np.flatnonzero(c0.op == 10)
    cps = [int(at[20]) + 1, int(at[41]), c0.n_gates]  # behind a channel gate, in front of one, the whole program
    kw = dict(seed=SEED, state_index=STATE_INDEX, trajectory=TRAJECTORY)
    with gpu_ctx.build_mps_scan(circuits, cps, **kw) as scan:
        final = scan.states(-1)
        for a, b in zip(final, dev):  # the snapshots are copies: the run is the run without them
            assert same_bits(a, b)
        for j, cp in enumerate(cps[:-1]):
            snap, done = scan.states(j), int(np.count_nonzero(at < cp))
            assert np.array_equal(scan.info(j)["logw"], [m.logw for m in snap])
            for m, f in zip(snap, final):
                assert np.array_equal(m.branches, f.branches[:done]) and m.logw != f.logw
            with gpu_ctx.build_mps_scan([c.sliced(cp, c.n_gates) for c in circuits], [c0.n_gates - cp], initial=(scan, j), **kw) as resumed:
                assert resumed.first_gate == cp
                for a, b in zip(resumed.states(-1), final):  # an interrupted run draws what the uninterrupted one draws
                    assert a.fidelity == b.fidelity and a.logw == b.logw and np.array_equal(a.branches, b.branches[done:])
                    assert all(np.array_equal(x, y) for x, y in zip(a.tensors, b.tensors))
            with gpu_ctx.build_mps_scan([c.sliced(cp, c.n_gates) for c in circuits], [c0.n_gates - cp], initial=(scan, j), first_gate=0, **kw) as wrong:
                assert any(not np.array_equal(a.branches, b.branches[done:]) for a, b in zip(wrong.states(-1), final))  # other counters, other draws


def test_resume_into_a_tail_without_channel_gates_keeps_logw(gpu_ctx):
    """Two noisy layers, then a layer without noise: a build resumed behind the last channel gate runs no code 10, and its records
    carry the log-weight of the snapshot -- with the tail's channel table (the channel entry) and without one (the plain entry)."""
    from qml_cutensornet_amd.engine import with_noise

    n, kw = 8, dict(seed=SEED, state_index=np.array([5, 6]), trajectory=np.array([1, 0]))
    circuits, cp = [], None
    for x in features(2, n, 43):
        head = with_noise(brickwork(n, 2, x, seed=3), "AmplitudeDamping", [0.1], after="two_qubit")
        circuits.append(from_gates(n, head + brickwork(n, 1, x, seed=4)))
        cp = from_gates(n, head).n_gates
    c0 = circuits[0]
    assert np.array_equal(c0.op[:cp], from_gates(n, head).op) and (c0.op[:cp] == 10).any() and not (c0.op[cp:] == 10).any() and (c0.op[cp:] == 9).any()
    with gpu_ctx.build_mps_scan(circuits, [cp, c0.n_gates], max_bond=64, **kw) as scan:
        final, logw = scan.states(-1), scan.info(0)["logw"]
        assert np.all(logw < 0) and np.array_equal(scan.info(-1)["logw"], logw) and [m.logw for m in final] == logw.tolist()
        tails = [c.sliced(cp, c.n_gates) for c in circuits]
        bare = [dataclasses.replace(c, channel=None, branch=None, kraus=None, n_kraus=None) for c in tails]
        for tail in (tails, bare):
            with gpu_ctx.build_mps_scan(tail, [c0.n_gates - cp], max_bond=64, initial=(scan, 0), **kw) as resumed:
                assert np.array_equal(resumed.info(-1)["logw"], logw) and resumed.info(-1)["branches"].shape == (2, 0)
                for a, b in zip(resumed.states(-1), final):
                    assert a.logw == b.logw and a.fidelity == b.fidelity and all(np.array_equal(x, y) for x, y in zip(a.tensors, b.tensors))


def test_at_bond_cap_64_a_state_does_not_depend_on_the_size_of_its_set(gpu_ctx, monkeypatch):
    """max_bond in 33 .. 64 is where a program without channels picks its workgroup shape by the number of states (512 threads for
    at most one state per CU, else 256).  A program of trajectories must not: its shape follows from max_bond alone, so a state
    built alone has the bits it has under QK_BUILD_WGS=2, the shape of a set larger than the device, and the bits it has in a set."""
    x = features(3, 12, 41)
    circuits = [from_gates(12, noisy_12_gates(x[k], measure=False)) for k in (1, 0, 1)]
    kw = dict(max_bond=64, seed=SEED)
    alone, info = gpu_ctx.build_mps([circuits[0]], state_index=0, trajectory=0, **kw)
    assert alone[0].max_bond() == 64 and alone[0].logw < 0
    assert info["threads"] == 256 and info["grid"] == 1  # one state, and still the 256-thread shape
    some, _ = gpu_ctx.build_mps(circuits, state_index=np.array([0, 1, 0]), trajectory=np.array([0, 0, 3]), **kw)
    assert same_bits(alone[0], some[0])
    monkeypatch.setenv("QK_BUILD_WGS", "2")
    pinned, pinned_info = gpu_ctx.build_mps([circuits[0]], state_index=0, trajectory=0, **kw)
    assert same_bits(alone[0], pinned[0])
    assert (pinned_info["threads"], pinned_info["slots"]) == (info["threads"], info["slots"])  # the shape it took on its own is the two-workgroup one


def test_capped_device_build_with_channels(gpu_ctx, noisy_12):
    import qml_cutensornet_amd as Q

    circuits, _, _ = noisy_12
    host, margin = [], np.inf
    for c, s, t in zip(circuits, STATE_INDEX, TRAJECTORY):
        m, mg = Q.simulate(c, 1 - 1e-16, max_bond=8, seed=SEED, state_index=int(s), trajectory=int(t), margin=True)
        host.append(m)
        margin = min(margin, mg)
    assert margin >= 1e-6
    dev, info = gpu_ctx.build_mps(circuits, max_bond=8, truncate=True, seed=SEED, state_index=STATE_INDEX, trajectory=TRAJECTORY)
    assert not info["dropped"]
    for d, h in zip(dev, host):
        print(f"capped at 8: device fidelity {d.fidelity:.15e}, host {h.fidelity:.15e}, difference {d.fidelity - h.fidelity:.3e}; logw {d.logw:.12f} / {h.logw:.12f}")
        assert np.array_equal(d.branches, h.branches)
        assert d.max_bond() <= 8 and d.bond_dims().max() == 8 and d.fidelity < 1 - 1e-3
        assert abs(d.fidelity - h.fidelity) < 1e-9 * max(1.0, h.fidelity)


@pytest.mark.parametrize("case", range(1, N_BAD_CHANNELS + 1))
def test_device_entry_rejects_bad_channel_gates(gpu_ctx, case):
    """The list of tests/test_channels_host.py through ``qk_build_mps_channels``: each a QkError raised by the checks in front of the
    launch, naming the gate's position."""
    from qml_cutensornet_amd.engine import QkError

    progs = bad_channel_programs()
    label, c, text = progs[case]
    with pytest.raises(QkError, match=text):
        gpu_ctx.build_mps([c, c])


def test_device_entry_accepts_the_good_programs_and_names_an_impossible_outcome(gpu_ctx):
    from qml_cutensornet_amd.engine import QkError

    progs = bad_channel_programs()
    dev, info = gpu_ctx.build_mps([progs[0][1], progs[0][1]], seed=3)
    assert info["branches"].shape == (2, 2) and abs(dev[0].fidelity - 1) < 1e-12
    forced, info = gpu_ctx.build_mps([progs[-1][1]])  # a forced branch may be any finite matrix
    assert info["branches"].tolist() == [[1, 0]]
    ok = from_gates(3, [("H", [0], []), ("X", [2], []), ("CX", [0, 1], []), ("PostSelect", [2], [1])])
    bad = ok.with_branches([0])
    dev, _ = gpu_ctx.build_mps([ok, ok], state_index=np.array([7, 9]))
    assert dev[1].logw == 0.0
    with pytest.raises(QkError, match=r"state 1 \(state_index 9\), gate 3"):
        gpu_ctx.build_mps([ok, bad], state_index=np.array([7, 9]))
    with pytest.raises(QkError, match="share their gate structure"):
        gpu_ctx.build_mps([ok, dataclasses.replace(ok, kraus=ok.kraus * 1.0 + 0.0, channel=np.where(ok.channel >= 0, ok.channel, -2).astype(np.int32))])


# ---- the two drivers
def noisy_ansatz(n=8):
    import qml_cutensornet_amd as Q
    from qml_cutensornet_amd.engine import with_noise

    return Q.CircuitAnsatz(n, with_noise(zz_template(n, 2, 0.8, 2), "AmplitudeDamping", [0.05], after="two_qubit"))


def _bloch(v, n):
    psi = v.reshape((2,) * n)
    out = np.zeros((n, 3))
    for k in range(n):
        m = np.moveaxis(psi, k, 0).reshape(2, -1)
        rho = m @ m.conj().T / np.vdot(v, v).real
        out[k] = [2 * rho[0, 1].real, -2 * rho[0, 1].imag, (rho[0, 0] - rho[1, 1]).real]  # <X>, <Y>, <Z>
    return out


def _host_trajectories(ans, P, first, T, seed):
    import qml_cutensornet_amd as Q

    vecs, margin = [], np.inf
    for p, x in enumerate(P):
        row = []
        for t in range(T):
            m, mg = Q.simulate(ans.circuit_for_data(x), 1 - 1e-16, seed=seed, state_index=first + p, trajectory=t, margin=True)
            row.append(mps_vector(m))
            margin = min(margin, mg)
        vecs.append(row)
    return vecs, margin


@pytest.fixture(scope="module")
def driver_reference(built):
    n, T, seed = 8, 3, 5
    ans = noisy_ansatz(n)
    X, Y = R.synthetic_features(4, n, 13), R.synthetic_features(3, n, 14)
    vx, mx = _host_trajectories(ans, X, 0, T, seed)
    vy, my = _host_trajectories(ans, Y, len(X), T, seed)  # Y after X
    return n, T, seed, ans, X, Y, vx, vy, min(mx, my)


@pytest.mark.parametrize("builder", ["device", "host"])
def test_noisy_kernel_drivers_against_host_mirror_trajectories(built, driver_reference, monkeypatch, builder):
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_noisy_kernel_matrix, build_noisy_projected_kernel_matrix

    monkeypatch.setenv("QK_BUILDER", builder)
    n, T, seed, ans, X, Y, vx, vy, margin = driver_reference
    assert margin >= 1e-6
    fx = np.array([np.mean([_bloch(v, n) for v in row], axis=0) for row in vx])
    fy = np.array([np.mean([_bloch(v, n) for v in row], axis=0) for row in vy])
    g = 1.0 / n

    def pqk(a, b):
        return np.exp(-0.5 * g * ((b[:, None] - a[None, :]) ** 2).sum(axis=(2, 3)))

    K = build_noisy_projected_kernel_matrix(SingleComm(), ans, X, trajectories=T, noise_seed=seed, truncation_error=1e-16)
    assert K.shape == (4, 4) and np.abs(K - pqk(fx, fx)).max() < 1e-9
    Kt = build_noisy_projected_kernel_matrix(SingleComm(), ans, X, Y=Y, trajectories=T, noise_seed=seed, truncation_error=1e-16)
    assert Kt.shape == (3, 4) and np.abs(Kt - pqk(fx, fy)).max() < 1e-9
    # rdm = 2: the pair correlators of the trajectory-averaged state, every pair up to distance 2 (the reshape over (point, T))
    D = 2
    tx = np.array([np.mean([pair_dist_from_dense(v, n, D)[0] for v in row], axis=0) for row in vx])
    ty = np.array([np.mean([pair_dist_from_dense(v, n, D)[0] for v in row], axis=0) for row in vy])
    K2 = build_noisy_projected_kernel_matrix(SingleComm(), ans, X, trajectories=T, noise_seed=seed, rdm=2, pair_distance=D, truncation_error=1e-16)
    assert K2.shape == (4, 4) and np.abs(K2 - ref_pair_gram(tx, tx, 1.0 / (n * D))).max() < 1e-9
    K2t = build_noisy_projected_kernel_matrix(SingleComm(), ans, X, Y=Y, trajectories=T, noise_seed=seed, rdm=2, pair_distance=D, pqk_gamma=0.2, truncation_error=1e-16)
    assert K2t.shape == (3, 4) and np.abs(K2t - ref_pair_gram(tx, ty, 0.2)).max() < 1e-9

    def fid(a, b, same):
        out = np.zeros((len(b), len(a)))
        for j, rb in enumerate(b):
            for i, ra in enumerate(a):
                o = np.array([[abs(np.vdot(p, q)) ** 2 for p in ra] for q in rb])
                out[j, i] = (o.sum() - np.trace(o)) / (T * (T - 1)) if same and i == j else o.mean()
        return out

    F = build_noisy_kernel_matrix(SingleComm(), ans, X, trajectories=T, noise_seed=seed, truncation_error=1e-16)
    assert F.shape == (4, 4) and np.abs(F - fid(vx, vx, True)).max() < 1e-9 and F.diagonal().max() < 1 - 1e-6  # purities of mixed states
    Ft = build_noisy_kernel_matrix(SingleComm(), ans, X, Y=Y, trajectories=T, noise_seed=seed, truncation_error=1e-16)
    assert Ft.shape == (3, 4) and np.abs(Ft - fid(vx, vy, False)).max() < 1e-9
    with pytest.raises(ValueError, match="trajectories >= 2"):
        build_noisy_kernel_matrix(SingleComm(), ans, X, trajectories=1, truncation_error=1e-16)


def test_one_trajectory_without_channels_is_the_noiseless_call(built, monkeypatch):
    import qml_cutensornet_amd as Q
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import (build_kernel_matrix, build_noisy_kernel_matrix, build_noisy_projected_kernel_matrix,
                                                                    build_projected_kernel_matrix)

    monkeypatch.setenv("QK_BUILDER", "device")
    n = 8
    ans = Q.CircuitAnsatz(n, zz_template(n, 2, 0.8, 2))
    X = R.synthetic_features(4, n, 13)
    a = build_noisy_kernel_matrix(SingleComm(), ans, X, trajectories=1, truncation_error=1e-16)
    assert np.abs(a - build_kernel_matrix(SingleComm(), ans, X=X, truncation_error=1e-16)).max() < 1e-12
    b = build_noisy_projected_kernel_matrix(SingleComm(), ans, X, trajectories=1, rdm=2, pair_distance=2, truncation_error=1e-16)
    assert np.abs(b - build_projected_kernel_matrix(SingleComm(), ans, X, rdm=2, pair_distance=2, truncation_error=1e-16)).max() < 1e-12


def test_drivers_without_trajectories_reject_drawn_channels(built):
    """The drivers from before the channels build a share without a seed and with rank-local positions: a drawn channel is refused."""
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_kernel_matrix, build_projected_kernel_matrix

    ans, X = noisy_ansatz(8), R.synthetic_features(2, 8, 13)
    with pytest.raises(ValueError, match="drawn Kraus channels"):
        build_kernel_matrix(SingleComm(), ans, X=X, truncation_error=1e-16)
    with pytest.raises(ValueError, match="drawn Kraus channels"):
        build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16)


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["QK_BUILDER"] = "host"
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oracle import restatement as R_
        from qml_cutensornet_amd.dist import TorchComm
        from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_noisy_kernel_matrix, build_noisy_projected_kernel_matrix
        from test_gpu_channels import noisy_ansatz as ansatz_

        ans = ansatz_(8)
        X, Y = R_.synthetic_features(4, 8, 13), R_.synthetic_features(3, 8, 14)
        comm = TorchComm()
        out = {"pqk": build_noisy_projected_kernel_matrix(comm, ans, X, Y=Y, trajectories=3, noise_seed=5, truncation_error=1e-16),
               "fid": build_noisy_kernel_matrix(comm, ans, X, trajectories=3, noise_seed=5, truncation_error=1e-16)}
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_match_one_rank_bitwise(built, monkeypatch):
    import torch.multiprocessing as mp

    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_noisy_kernel_matrix, build_noisy_projected_kernel_matrix

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + ((os.getpid() + 1361) % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert res[1]["pqk"] is None and res[1]["fid"] is None
    monkeypatch.setenv("QK_BUILDER", "host")
    ans = noisy_ansatz(8)
    X, Y = R.synthetic_features(4, 8, 13), R.synthetic_features(3, 8, 14)
    assert np.array_equal(res[0]["pqk"], build_noisy_projected_kernel_matrix(SingleComm(), ans, X, Y=Y, trajectories=3, noise_seed=5, truncation_error=1e-16))
    assert np.array_equal(res[0]["fid"], build_noisy_kernel_matrix(SingleComm(), ans, X, trajectories=3, noise_seed=5, truncation_error=1e-16))


# ---- a program without channels: the bits of the build before op code 10 existed
def parent_program():
    import qml_cutensornet_amd as Q

    ans = Q.CircuitAnsatz(12, zz_template(12, 2, 0.8, 3))
    return [ans.circuit_for_data(x) for x in R.synthetic_features(4, 12, 7)]


def state_digests(states):
    return [{"dims": [int(d) for d in m.bond_dims()], "fidelity": float(m.fidelity).hex(),
             "sha256": hashlib.sha256(b"".join(np.ascontiguousarray(t, dtype=np.complex128).tobytes() for t in m.tensors)).hexdigest()} for m in states]


def test_a_program_without_channels_downloads_the_bits_of_the_parent_build(gpu_ctx):
    """tests/golden/channels_parent_bits.json was recorded once with ``state_digests(gpu_ctx.build_mps(parent_program())[0])`` from the
    commit before this op code was added."""
    circuits = parent_program()
    assert set(circuits[0].op.tolist()) == {0, 1, 3, 4, 5, 6, 7}  # every named gate kind of the template, SWAP chains included
    with open(os.path.join(ROOT, "tests", "golden", "channels_parent_bits.json")) as fp:
        want = json.load(fp)
    dev, info = gpu_ctx.build_mps(circuits)
    assert state_digests(dev) == want["states"]
    assert info["branches"].shape == (4, 0) and not info["logw"].any()
    table = bad_channel_programs()[0][1]
    none = np.full(circuits[0].op.shape, -1, dtype=np.int32)
    through_new_entry, _ = gpu_ctx.build_mps([dataclasses.replace(c, channel=none, branch=none, kraus=table.kraus, n_kraus=table.n_kraus) for c in circuits], seed=9)
    assert state_digests(through_new_entry) == want["states"]
