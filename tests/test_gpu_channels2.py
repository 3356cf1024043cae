"""GPU tests of the two-qubit Kraus channels (op code 11) in the device builder: a noisy Haar brickwork with Depolarizing2q behind
every two-qubit gate and a mid-circuit Measure2q against the host builder in the one- and two-workgroup shapes, the same circuit
capped at bond 32 in the four-workgroup shape (where the LDS staging is tightest), the 32-branch exact enumeration as one call,
replay (the two-accumulator path of forced branches), independence of a state from its set, snapshots and resume, the rejections and
the run-time error of ``qk_build_mps_channels2``, the refusal of a launch shape whose LDS cannot hold the staging, the two noisy
kernel drivers, and the bits of programs without code 11 against the build before this op code existed
(tests/golden/channels_parent_bits.json, tests/golden/channels2_parent_bits.json).

Tolerances as tests/test_gpu_channels.py: fidelity within 1e-12 of 1, |<dev|host>|^2 = 1 within 1e-10, the capped build
|f_dev - f_host| < 1e-9 max(1, f_host); log-weights within 1e-10, the dense density matrix within 1e-10, the drivers within 1e-9.
Device and host draw the same branches when no draw of the host sits within 1e-6 of a threshold: asserted first, a condition of the
comparison, not a measurement."""
import dataclasses
import json
import math
import os

import numpy as np
import pytest

from oracle import restatement as R
from test_channels2_host import ENUM2_BRANCHES, ENUM2_GATES, N_BAD_CHANNELS2, bad_channel2_programs, dense_rho2
from test_feature_map_host import zz_template
from test_gpu_channels import EXTRAS, _bloch, noisy_12_gates, parent_program, same_bits, state_digests
from test_matrix_gates_host import brickwork, features, from_gates, mps_vector

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 2024
STATE_INDEX = np.array([0, 0, 1, 1, 2, 2])
TRAJECTORY = np.array([0, 1, 0, 1, 0, 1])


def noisy2_12_gates(x):
    """n = 12: the six-layer Haar brickwork of tests/test_gpu_channels.py, Depolarizing2q(0.05) behind every two-qubit gate on its
    pair (16 matrices, drawn) and a Measure2q (4, drawn) in mid-chain after the third layer."""
    from qml_cutensornet_amd.engine import with_noise

    n = 12
    first, rest = brickwork(n, 3, x, seed=17), brickwork(n, 6, x, seed=17, extras=EXTRAS)
    gates = rest[: len(first)] + [("Measure2q", [5, 6], [])] + rest[len(first):]
    return with_noise(gates, "Depolarizing2q", [0.05], after="two_qubit")


def host_states(circuits, **kw):
    import qml_cutensornet_amd as Q

    host, margin = [], np.inf
    for c, s, t in zip(circuits, STATE_INDEX, TRAJECTORY):
        m, mg = Q.simulate(c, 1 - 1e-16, seed=SEED, state_index=int(s), trajectory=int(t), margin=True, **kw)
        host.append(m)
        margin = min(margin, mg)
    return host, margin


@pytest.fixture(scope="module")
def noisy2_12(built):
    """3 states x 2 trajectories: (circuits, host states, host margin)."""
    circuits = [from_gates(12, noisy2_12_gates(x)) for x in features(3, 12, 41) for _ in range(2)]
    return (circuits,) + host_states(circuits)


@pytest.fixture(scope="module")
def dev2_12(gpu_ctx, noisy2_12):
    return gpu_ctx.build_mps(noisy2_12[0], seed=SEED, state_index=STATE_INDEX, trajectory=TRAJECTORY)


@pytest.mark.parametrize("wgs", ["1", "2"])
def test_device_builder_matches_host_builder_on_a_noisy_brickwork(gpu_ctx, noisy2_12, monkeypatch, wgs):
    monkeypatch.setenv("QK_BUILD_WGS", wgs)
    circuits, host, margin = noisy2_12
    c0 = circuits[0]
    assert c0.n_channel_gates == int(np.count_nonzero(c0.op == 9)) + 1 == int(np.count_nonzero(c0.op == 11)) and sorted(set(c0.n_kraus2.tolist())) == [4, 16]
    assert margin >= 1e-6  # the condition of the comparison (another SEED if it ever fails)
    dev, info = gpu_ctx.build_mps(circuits, seed=SEED, state_index=STATE_INDEX, trajectory=TRAJECTORY)
    print(f"two-qubit channels, n = 12, six Haar layers, {c0.n_channel_gates} channel gates, 6 states, QK_BUILD_WGS={wgs}: kernel_ms = {info['kernel_ms']:.3f}")
    # theta of every size class: l r below the block, no multiple of it, mid below and from 32 on
    assert max(m.max_bond() for m in host) >= 32 and min(m.bond_dims()[1:-1].min() for m in host) <= 2
    assert info["branches"].shape == (6, c0.n_channel_gates) and info["branches"].min() >= 0
    for s, (md, mh) in enumerate(zip(dev, host)):
        assert np.array_equal(md.branches, mh.branches) and np.array_equal(info["branches"][s], mh.branches)
        assert np.array_equal(md.bond_dims(), mh.bond_dims())
        assert abs(abs(R.mps_inner(md.tensors, mh.tensors)) ** 2 - 1) < 1e-10
        assert abs(md.logw - mh.logw) < 1e-10 and info["logw"][s] == md.logw
        assert abs(md.fidelity - 1.0) < 1e-12
    assert len({tuple(m.branches.tolist()) for m in dev}) > 1  # the trajectories differ


def test_four_workgroup_shape_capped_at_bond_32(gpu_ctx, noisy2_12, monkeypatch):
    """QK_BUILD_WGS=4: 38 KiB of LDS per workgroup, the shape the grouping of the Kraus matrices is made for.  The Measure2q in
    mid-chain keeps the bonds of this circuit at 32, so the cap admits the shape and cuts nothing: beside the checks of the capped
    build, the states are those of the host."""
    circuits = noisy2_12[0]
    monkeypatch.setenv("QK_BUILD_WGS", "1")
    cus = gpu_ctx.build_mps(circuits[:1], max_bond=32, truncate=True, seed=SEED, state_index=STATE_INDEX[:1], trajectory=TRAJECTORY[:1])[1]["slots"]  # one workgroup per CU
    monkeypatch.setenv("QK_BUILD_WGS", "4")
    host, margin = host_states(circuits, max_bond=32)
    assert margin >= 1e-6 and all(h.max_bond() == 32 and h.fidelity == 1.0 for h in host)
    dev, info = gpu_ctx.build_mps(circuits, max_bond=32, truncate=True, seed=SEED, state_index=STATE_INDEX, trajectory=TRAJECTORY)
    print(f"two-qubit channels capped at 32, QK_BUILD_WGS=4: kernel_ms = {info['kernel_ms']:.3f}")
    assert not info["dropped"]
    assert info["threads"] == 256 and info["slots"] == 4 * cus and info["grid"] == len(circuits)  # the launch record: the four-workgroup shape
    for d, h in zip(dev, host):
        print(f"capped at 32: device fidelity {d.fidelity:.15e}, host {h.fidelity:.15e}, difference {d.fidelity - h.fidelity:.3e}; logw {d.logw:.12f} / {h.logw:.12f}")
        assert np.array_equal(d.branches, h.branches)
        assert d.max_bond() <= 32 and d.bond_dims().max() == 32 and abs(d.fidelity - h.fidelity) < 1e-9 * max(1.0, h.fidelity)
        assert np.array_equal(d.bond_dims(), h.bond_dims()) and abs(abs(R.mps_inner(d.tensors, h.tensors)) ** 2 - 1) < 1e-10 and abs(d.logw - h.logw) < 1e-10


def test_capped_device_build_with_two_qubit_channels(gpu_ctx, noisy2_12):
    circuits = noisy2_12[0]
    host, margin = host_states(circuits, max_bond=8)
    assert margin >= 1e-6
    dev, info = gpu_ctx.build_mps(circuits, max_bond=8, truncate=True, seed=SEED, state_index=STATE_INDEX, trajectory=TRAJECTORY)
    assert not info["dropped"]
    for d, h in zip(dev, host):
        assert np.array_equal(d.branches, h.branches)
        assert d.max_bond() <= 8 and d.bond_dims().max() == 8 and d.fidelity < 1 - 1e-3
        assert abs(d.fidelity - h.fidelity) < 1e-9 * max(1.0, h.fidelity)


def test_exact_enumeration_on_the_device(gpu_ctx):
    """The n = 6 case of the host tests as 32 states of one call with per-state forced branches."""
    n = 6
    c = from_gates(n, ENUM2_GATES)
    dev, info = gpu_ctx.build_mps([c.with_branches(r) for r in ENUM2_BRANCHES])
    assert info["branches"].tolist() == [list(r) for r in ENUM2_BRANCHES]
    rho, total = np.zeros((2 ** n, 2 ** n), dtype=complex), 0.0
    for m in dev:
        v = mps_vector(m)
        assert abs(np.vdot(v, v).real - 1) < 1e-12
        rho += math.exp(m.logw) * np.outer(v, v.conj())
        total += math.exp(m.logw)
    assert abs(total - 1) < 1e-10 and np.abs(rho - dense_rho2(n, ENUM2_GATES)).max() < 1e-10


def test_replay_and_run_to_run_are_bit_identical(gpu_ctx, noisy2_12, dev2_12):
    """The replay forces every branch: one pass with two sums (N and p_b) instead of the groups of four -- the same bits."""
    circuits = noisy2_12[0]
    dev, _ = dev2_12
    again, _ = gpu_ctx.build_mps(circuits, seed=SEED, state_index=STATE_INDEX, trajectory=TRAJECTORY)
    replay, _ = gpu_ctx.build_mps([c.with_branches(m.branches) for c, m in zip(circuits, dev)], seed=SEED + 1, state_index=STATE_INDEX[::-1].copy())
    for a, b, c in zip(dev, again, replay):
        assert same_bits(a, b) and same_bits(a, c)


def test_a_state_does_not_depend_on_its_set(gpu_ctx, noisy2_12, dev2_12):
    circuits = noisy2_12[0]
    dev, _ = dev2_12
    alone, _ = gpu_ctx.build_mps([circuits[3]], seed=SEED, state_index=int(STATE_INDEX[3]), trajectory=int(TRAJECTORY[3]))
    assert same_bits(alone[0], dev[3])
    order = [4, 1, 5]  # other states, another order
    some, _ = gpu_ctx.build_mps([circuits[k] for k in order], seed=SEED, state_index=STATE_INDEX[order], trajectory=TRAJECTORY[order])
    for m, k in zip(some, order):
        assert same_bits(m, dev[k])
    other, _ = gpu_ctx.build_mps([circuits[3]], seed=SEED, state_index=int(STATE_INDEX[3]), trajectory=7)
    assert not np.array_equal(other[0].branches, dev[3].branches)  # (34 draws: another trajectory is another sequence at this seed)


def test_snapshots_and_resume_with_first_gate(gpu_ctx, noisy2_12, dev2_12):
    circuits = noisy2_12[0]
    dev, _ = dev2_12
    c0 = circuits[0]
    at = np.flatnonzero(c0.op == 11)
    cps = [int(at[10]) + 1, int(at[21]), c0.n_gates]  # behind a channel gate, in front of one, the whole program
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


def test_a_program_mixing_both_codes_matches_the_host(gpu_ctx):
    from test_channels2_host import mixed_gates

    import qml_cutensornet_amd as Q

    c = from_gates(5, mixed_gates())
    idx = np.arange(6)
    host = [Q.simulate(c, 1 - 1e-16, seed=21, state_index=int(s), margin=True) for s in idx]
    assert min(mg for _, mg in host) >= 1e-6
    dev, info = gpu_ctx.build_mps([c] * 6, seed=21, state_index=idx)
    assert info["branches"].shape == (6, 6)
    for d, (h, _) in zip(dev, host):
        assert np.array_equal(d.branches, h.branches) and abs(d.logw - h.logw) < 1e-10 and abs(abs(R.mps_inner(d.tensors, h.tensors)) ** 2 - 1) < 1e-10


@pytest.mark.parametrize("case", range(1, N_BAD_CHANNELS2 + 1))
def test_device_entry_rejects_bad_two_qubit_channel_gates(gpu_ctx, case):
    """The list of tests/test_channels2_host.py through ``qk_build_mps_channels2``: each a QkError raised by the checks in front of
    the launch, naming the gate's position."""
    from qml_cutensornet_amd.engine import QkError

    label, c, text = bad_channel2_programs()[case]
    with pytest.raises(QkError, match=text):
        gpu_ctx.build_mps([c, c])


def test_device_entry_accepts_the_good_programs_and_names_an_impossible_outcome(gpu_ctx, monkeypatch):
    from qml_cutensornet_amd.engine import QkError

    progs = bad_channel2_programs()
    dev, info = gpu_ctx.build_mps([progs[0][1], progs[0][1]], seed=3)
    assert info["branches"].shape == (2, 3) and abs(dev[0].fidelity - 1) < 1e-12
    forced, info = gpu_ctx.build_mps([progs[-1][1]], seed=1)  # a forced branch may be any finite matrix
    assert info["branches"].tolist()[0][:2] == [7, 0]
    ok = from_gates(3, [("H", [1], []), ("CX", [1, 2], []), ("Ry", [0], [0.3]), ("PostSelect2q", [1, 2], [3])])
    bad = ok.with_branches([1])  # |00> + |11> has no weight on 01
    dev, _ = gpu_ctx.build_mps([ok, ok], state_index=np.array([7, 9]))
    assert abs(dev[1].logw - math.log(0.5)) < 1e-14 and dev[1].bond_dims().max() == 1  # the bond of the Bell pair shrank
    with pytest.raises(QkError, match=r"state 1 \(state_index 9\), gate 3"):
        gpu_ctx.build_mps([ok, bad], state_index=np.array([7, 9]))
    with pytest.raises(QkError, match="share their gate structure"):
        gpu_ctx.build_mps([ok, dataclasses.replace(ok, kraus2=ok.kraus2 * 1.0 + 0.0, channel=np.where(ok.channel >= 0, ok.channel, -2).astype(np.int32))])
    # 64 staged complex numbers, five partials per thread, N and sixteen p_k: 713 complex numbers at 256 threads.  32 KiB of LDS
    # (the smallest QK_BUILD_LDS_KB admits) hold them behind the bond tables of max_bond 256; behind those of max_bond 1000
    # (24016 bytes) 547 complex numbers are left: refused by the host check in front of the launch, nothing is allocated or run.
    monkeypatch.setenv("QK_BUILD_WGS", "4")
    monkeypatch.setenv("QK_BUILD_LDS_KB", "32")
    dev, _ = gpu_ctx.build_mps([ok], state_index=7)
    assert abs(dev[0].logw - math.log(0.5)) < 1e-14
    with pytest.raises(QkError, match="two-qubit channel step needs 713 complex numbers of LDS working set, this shape leaves 547"):
        gpu_ctx.build_mps([ok], state_index=7, max_bond=1000)


# ---- the two drivers
def noisy2_ansatz(n=8):
    import qml_cutensornet_amd as Q
    from qml_cutensornet_amd.engine import with_noise

    return Q.CircuitAnsatz(n, with_noise(zz_template(n, 2, 0.8, 2), "Depolarizing2q", [0.1], after="two_qubit"))


@pytest.mark.parametrize("builder", ["device", "host"])
def test_noisy_kernel_drivers_against_host_mirror_trajectories(built, monkeypatch, builder):
    import qml_cutensornet_amd as Q
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_noisy_kernel_matrix, build_noisy_projected_kernel_matrix

    monkeypatch.setenv("QK_BUILDER", builder)
    n, T, seed = 8, 3, 8  # (a seed whose host draws all keep the margin asserted below)
    ans = noisy2_ansatz(n)
    assert ans.circuit_for_data(np.zeros(n)).n_channel_gates > 0 and ans.ansatz_circ.kraus is None
    X = R.synthetic_features(4, n, 13)
    vx, margin = [], np.inf
    for p, x in enumerate(X):
        row = []
        for t in range(T):
            m, mg = Q.simulate(ans.circuit_for_data(x), 1 - 1e-16, seed=seed, state_index=p, trajectory=t, margin=True)
            row.append(mps_vector(m))
            margin = min(margin, mg)
        vx.append(row)
    assert margin >= 1e-6
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
    assert F.shape == (4, 4) and np.abs(F - ref).max() < 1e-9 and F.diagonal().max() < 1 - 1e-6  # purities of mixed states


def test_drivers_without_trajectories_reject_drawn_two_qubit_channels(built):
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_kernel_matrix

    with pytest.raises(ValueError, match="drawn Kraus channels"):
        build_kernel_matrix(SingleComm(), noisy2_ansatz(8), X=R.synthetic_features(2, 8, 13), truncation_error=1e-16)


# ---- programs without code 11: the bits of the build before this op code existed
def code10_program():
    """Four states of the noisy 12-qubit circuit of tests/test_gpu_channels.py (code 10 only), with their trajectory names."""
    return [from_gates(12, noisy_12_gates(x)) for x in features(2, 12, 41) for _ in range(2)], dict(seed=SEED, state_index=np.array([0, 0, 1, 1]), trajectory=np.array([0, 1, 0, 1]))


def trajectory_digests(states):
    return [dict(d, logw=float(m.logw).hex(), branches=m.branches.tolist()) for d, m in zip(state_digests(states), states)]


def test_programs_without_code_11_download_the_bits_of_the_parent_build(gpu_ctx):
    """tests/golden/channels2_parent_bits.json was recorded once with ``trajectory_digests(gpu_ctx.build_mps(*code10_program())[0])``
    (the keyword arguments unpacked) from the commit before this op code was added; channels_parent_bits.json is older."""
    table = bad_channel2_programs()[0][1]
    plain = parent_program()
    with open(os.path.join(ROOT, "tests", "golden", "channels_parent_bits.json")) as fp:
        want = json.load(fp)
    assert state_digests(gpu_ctx.build_mps(plain)[0]) == want["states"]
    none = np.full(plain[0].op.shape, -1, dtype=np.int32)
    through_new_entry, _ = gpu_ctx.build_mps([dataclasses.replace(c, channel=none, branch=none, kraus2=table.kraus2, n_kraus2=table.n_kraus2) for c in plain], seed=9)
    assert state_digests(through_new_entry) == want["states"]
    circuits, kw = code10_program()
    assert set(circuits[0].op.tolist()) >= {9, 10} and 11 not in circuits[0].op
    from test_gpu_program_entry import BUILD_MPS, build_legacy, gate_program

    with_table = [dataclasses.replace(c, kraus2=table.kraus2, n_kraus2=table.n_kraus2) for c in circuits]
    with build_legacy(gpu_ctx, "qk_build_mps_channels", gate_program(circuits, **kw), **BUILD_MPS) as scan:  # the C entries themselves, through ctypes
        old = scan.states(0)
    with build_legacy(gpu_ctx, "qk_build_mps_channels2", gate_program(with_table, **kw), **BUILD_MPS) as scan:
        new = scan.states(0)
    for a, b, c, d in zip(old, new, gpu_ctx.build_mps(circuits, **kw)[0], gpu_ctx.build_mps(with_table, **kw)[0]):
        assert same_bits(a, b) and same_bits(a, c) and same_bits(a, d)
    with open(os.path.join(ROOT, "tests", "golden", "channels2_parent_bits.json")) as fp:
        want2 = json.load(fp)
    assert trajectory_digests(old) == want2["states"]
