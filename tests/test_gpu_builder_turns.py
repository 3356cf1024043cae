"""GPU tests of the device builder where a workgroup builds more than one state.  ``qk_build_kernel`` is persistent: it launches
min(n_states, slots) workgroups (slots = workgroups per CU x CUs) and a workgroup that has packed its state takes the next one from
the queue -- onto the arena, the workspaces, the LDS tables and the per-state locals of the state before.  Every build here holds
slots + 40 states (``helpers.BUILDER_TURN_SETS``; tests/test_builder_turns_host.py asserts what the cases are taken for), and every
test first asserts ``grid == slots < n_states`` and the threads of the shape from the launch record of the build (``info["grid"]``,
``info["threads"]``, ``info["slots"]``); the slots come from a probe build, not from a count of CUs.

References, for EVERY state of a build: (a) the host builder (``simulate_many``); (b) the same circuits built on the device in
chunks of at most slots // 2 states in the same pinned shape, where every state is the first of its workgroup.

Tolerances (those of tests/test_gpu_builder.py and tests/test_gpu_depth_scan.py, none measured on the code under test).  Against
(a): | |<dev|host>|^2 - 1 | < 1e-10 and |fidelity_dev - fidelity_host| < 1e-12 (the one build that truncates: see its test).  Against (b): equal bond tables, equal fidelity
bits and equal tensor bits when the builder repeats itself -- which ``reproducible`` checks first on two identical chunk builds of
the shape --, else equal bond tables, fidelity within 1e-12 and overlap defect below 1e-10.  Programs with channels (trajectories)
are bit-equal unconditionally: a trajectory's bits do not depend on what else the call builds.  Against the host's trajectories the
bounds of tests/test_gpu_channels.py, under its condition that no draw of the host sits within 1e-6 of a threshold."""
import contextlib
import dataclasses
import os

import numpy as np
import pytest

import helpers as H
from oracle import restatement as R
from test_channels2_host import noisy2_brickwork
from test_channels_host import noisy_brickwork
from test_feature_map_host import zz_template
from test_gpu_matrix_gates import _download
from test_matrix_gates_host import brickwork, features, from_gates, haar

pytestmark = pytest.mark.gpu

SEED = 2024


@contextlib.contextmanager
def _env(**kv):
    """os.environ with these values (None: unset) for the block; the module-scoped fixtures cannot take monkeypatch"""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _pinned(wgs, ordered=True):
    return _env(QK_BUILD_WGS=wgs, QK_BUILD_NO_ORDER=None if ordered else "1")


def _assert_turns(info, n_states, threads, per_cu, cus, what):
    """the precondition of every test here: the shape is the expected one (its threads, and per_cu workgroups on each of the CUs
    that ``cus`` counted), the grid is all of its slots, and there are more states than that"""
    print(f"{what}: {n_states} states on a grid of {info['grid']} x {info['threads']} threads ({info['slots']} slots), kernel_ms = {info.get('kernel_ms', float('nan')):.1f}")
    assert info["threads"] == threads and info["slots"] == per_cu * cus, (what, info["threads"], info["slots"], per_cu, cus)
    assert info["grid"] == info["slots"] < n_states, (what, info["grid"], info["slots"], n_states)


def _assert_first_turn(info, n_states, threads):
    assert info["grid"] == n_states <= info["slots"] // 2 and info["threads"] == threads


def _same_bits(a, b):
    return (a.fidelity == b.fidelity and a.logw == b.logw and np.array_equal(a.branches, b.branches) and np.array_equal(a.bond_dims(), b.bond_dims())
            and all(np.array_equal(s, t) for s, t in zip(a.tensors, b.tensors)))


def _defect(a, b):
    z = R.mps_inner(a.tensors, b.tensors)
    return abs(abs(z) ** 2 / (R.mps_inner(a.tensors, a.tensors).real * R.mps_inner(b.tensors, b.tensors).real) - 1.0)


def _assert_same(xs, ys, reproducible, what):
    """against reference (b): bit for bit -- or, on a builder that does not repeat itself, the weaker bounds of the docstring"""
    assert len(xs) == len(ys)
    for k, (a, b) in enumerate(zip(xs, ys)):
        assert (a is None) == (b is None), f"{what}: state {k}: dropped in one build only"
        if a is None:
            continue
        assert np.array_equal(a.bond_dims(), b.bond_dims()), f"{what}: state {k}: bond tables differ"
        if reproducible:
            assert _same_bits(a, b), f"{what}: state {k}: bits differ (fidelity {a.fidelity!r} / {b.fidelity!r})"
        else:
            assert abs(a.fidelity - b.fidelity) < 1e-12 and _defect(a, b) < 1e-10, f"{what}: state {k}"


def _assert_host(dev, host, what):
    """against reference (a)"""
    assert len(dev) == len(host)
    worst = 0.0
    for k, (d, h) in enumerate(zip(dev, host)):
        assert np.array_equal(d.bond_dims(), h.bond_dims()), f"{what}: state {k}: bonds {d.bond_dims()} / host {h.bond_dims()}"
        assert abs(d.fidelity - h.fidelity) < 1e-12, f"{what}: state {k}: fidelity {d.fidelity!r} / host {h.fidelity!r}"
        worst = max(worst, abs(abs(R.mps_inner(d.tensors, h.tensors)) ** 2 - 1))
        assert worst < 1e-10, f"{what}: state {k}: | |<dev|host>|^2 - 1 | = {worst:.3e}"
    print(f"{what}: {len(dev)} states against the host builder: largest | |<dev|host>|^2 - 1 | = {worst:.2e}")


def _chunks(n_states, slots):
    size = max(1, slots // 2)
    return [range(s0, min(n_states, s0 + size)) for s0 in range(0, n_states, size)]


def _build_in_chunks(ctx, circuits, slots, threads, **kw):
    """reference (b): (states, dropped), every state the first of its workgroup; per-state keywords (arrays) are cut with the chunks"""
    states, dropped = [], []
    for r in _chunks(len(circuits), slots):
        cut = {k: (v[r.start:r.stop] if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
        part, info = ctx.build_mps([circuits[i] for i in r], **cut)
        _assert_first_turn(info, len(r), threads)
        states += part
        dropped += [r.start + i for i in info["dropped"]]
    return states, dropped


class _Case:
    """one entry of helpers.BUILDER_TURN_SETS on this device: the circuits and both references"""

    def __init__(self, ctx, name, cus):
        self.name, self.cus = name, cus
        self.n, self.reps, self.d, self.max_bond, self.wgs, self.per_cu, self.threads, self.reach = H.BUILDER_TURN_SETS[name]
        with _pinned(self.wgs):
            _, probe = ctx.build_mps(H.builder_turn_circuits(name, 0, 2), max_bond=self.max_bond)
            assert probe["threads"] == self.threads and probe["grid"] == 2 and probe["slots"] == self.per_cu * cus
            self.slots = probe["slots"]
            self.circuits = H.builder_turn_circuits(name, self.slots)
            self.host = H.host_states(self.circuits)
            first = [self.circuits[i] for i in _chunks(len(self.circuits), self.slots)[0]]
            one, two = ctx.build_mps(first, max_bond=self.max_bond)[0], ctx.build_mps(first, max_bond=self.max_bond)[0]
            self.reproducible = all(_same_bits(a, b) for a, b in zip(one, two))
            print(f"{name}: two builds of the first chunk ({len(first)} states) are {'the same bits' if self.reproducible else 'NOT the same bits'}")
            self.chunked, _ = _build_in_chunks(ctx, self.circuits, self.slots, self.threads, max_bond=self.max_bond)
        self._big = None
        self.ctx = ctx

    def big(self):
        """the build of all slots + 40 states in the default order: (states, info)"""
        if self._big is None:
            with _pinned(self.wgs):
                self._big = self.ctx.build_mps(self.circuits, max_bond=self.max_bond)
            _assert_turns(self._big[1], len(self.circuits), self.threads, self.per_cu, self.cus, f"{self.name}, default order")
        return self._big


@pytest.fixture(scope="module")
def cus(gpu_ctx):
    """The CUs of the device: the slots of a build pinned to 512 threads, which holds one workgroup per CU.  Every other shape's
    slots are asserted to be its workgroups per CU times this."""
    with _pinned("1"):
        _, probe = gpu_ctx.build_mps(H.builder_turn_circuits("wide", 0, 2), max_bond=64)
    assert probe["threads"] == 512 and probe["grid"] == 2 and probe["slots"] >= 1
    return probe["slots"]


@pytest.fixture(scope="module")
def cases(gpu_ctx, cus):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Case(gpu_ctx, name, cus)
        return made[name]

    return get


# ---- 1. both queue orders, three shapes
@pytest.mark.parametrize("name", list(H.BUILDER_TURN_SETS))
def test_later_turn_states_in_the_default_order(cases, name):
    """Descending proxy: the 40 lightest states are built on workgroups that held heavier ones."""
    case = cases(name)
    dev, info = case.big()
    assert not info["dropped"]
    later = H.later_turn_states(case.circuits, case.slots)
    bonds = np.array([m.max_bond() for m in dev])
    assert len(later) == H.BUILDER_TURN_EXTRA and bonds[later].max() >= case.reach
    _assert_host(dev, case.host, f"{name}, default order")
    _assert_same(dev, case.chunked, case.reproducible, f"{name}, default order, against first-turn builds")


@pytest.mark.parametrize("name", list(H.BUILDER_TURN_SETS))
def test_later_turn_states_in_ascending_order(gpu_ctx, cases, name):
    """QK_BUILD_NO_ORDER with the circuits sorted by ascending proxy: the heaviest states come last, onto arenas that held light ones."""
    case = cases(name)
    up = H.ascending_by_proxy(case.circuits)
    with _pinned(case.wgs, ordered=False):
        dev, info = gpu_ctx.build_mps([case.circuits[i] for i in up], max_bond=case.max_bond)
    _assert_turns(info, len(up), case.threads, case.per_cu, case.cus, f"{name}, ascending order")
    assert not info["dropped"]
    bonds = np.array([m.max_bond() for m in dev])
    assert bonds[case.slots:].max() == bonds.max() >= case.reach and bonds[:case.slots].min() < bonds.max()
    _assert_host(dev, [case.host[i] for i in up], f"{name}, ascending order")
    _assert_same(dev, [case.chunked[i] for i in up], case.reproducible, f"{name}, ascending order, against first-turn builds")


def test_truncating_build_beyond_the_slots(gpu_ctx, cases):
    """``truncate=True`` at a cap that costs the first-turn states more than 1e-6 of fidelity (helpers.BUILDER_TURN_TRUNCATE): the
    fidelity product of a later-turn state starts from 1, not from what the state before it on its workgroup lost.  Against the host
    builder with the same cap the bounds of tests/test_gpu_builder.py::test_bond_cap_on_the_block_path -- same bonds, fidelity within
    1e-9 max(1, f_host), normalised overlap within 1e-9 of 1 --, which hold whether or not the builder repeats its bits; against the
    first-turn builds as everywhere here."""
    name, cap, share, least = H.BUILDER_TURN_TRUNCATE
    case = cases(name)
    host = H.host_states(case.circuits, max_bond=cap)
    with _pinned(case.wgs):
        dev, info = gpu_ctx.build_mps(case.circuits, max_bond=cap, truncate=True)
        _assert_turns(info, len(case.circuits), case.threads, case.per_cu, case.cus, f"{name} cut at bond {cap}")
        chunked, _ = _build_in_chunks(gpu_ctx, case.circuits, case.slots, case.threads, max_bond=cap, truncate=True)
    assert not info["dropped"]
    later = H.later_turn_states(case.circuits, case.slots)
    first = np.setdiff1d(np.arange(len(dev)), later)
    cut = np.array([m.fidelity < 1 - 1e-6 for m in dev])
    assert cut[first].sum() >= share * case.slots and cut[later].sum() >= least and (~cut[later]).sum() >= least
    for k, (d, h) in enumerate(zip(dev, host)):
        assert np.array_equal(d.bond_dims(), h.bond_dims()) and d.max_bond() <= cap, f"state {k}"
        assert abs(d.fidelity - h.fidelity) < 1e-9 * max(1.0, h.fidelity), f"state {k}: fidelity {d.fidelity!r} / host {h.fidelity!r}"
        assert _defect(d, h) < 1e-9, f"state {k}"
    _assert_same(dev, chunked, case.reproducible, f"{name} cut at bond {cap}, against first-turn builds")


# ---- 2. the whole vocabulary in the four-workgroup shape
def vocabulary_template(n):
    """Rz, Rx, Ry, ZZPhase up to distance 2 (SWAP routing, reversed pairs), YYPhase, constant angles (``zz_template``), and between
    its two layers a brickwork layer of Haar ``Unitary2q`` (every third pair reversed) with a ``Unitary1q`` on every second qubit."""
    rng = np.random.default_rng(29)
    consts = [(name, qs, ps[0]) for name, qs, ps in brickwork(n, 2, np.zeros(n), seed=17) if name == "Unitary2q"]
    consts += [("Unitary1q", [q], haar(rng, 2)) for q in range(0, n, 2)] + [("Unitary2q", [n - 1, n - 3], haar(rng, 4))]
    return zz_template(n, 1, 0.7, 2) + consts + zz_template(n, 1, 0.45, 2)


@pytest.fixture(scope="module")
def vocabulary(gpu_ctx, cases):
    import qml_cutensornet_amd as Q

    n, max_bond = 10, 32
    slots = cases("four").slots
    ans = Q.CircuitAnsatz(n, vocabulary_template(n))
    circuits = [ans.circuit_for_data(x) for x in R.synthetic_features(slots + H.BUILDER_TURN_EXTRA, n, 13)]
    with _pinned(None):
        dev, info = gpu_ctx.build_mps(circuits, max_bond=max_bond)
    return circuits, dev, info, slots


def test_whole_vocabulary_in_the_four_workgroup_shape(gpu_ctx, cases, cus, vocabulary):
    circuits, dev, info, slots = vocabulary
    assert {0, 1, 3, 4, 5, 6, 7, 8, 9} <= set(np.asarray(circuits[0].op).tolist())  # H, Rz, SWAP, Rx, Ry, YYPhase, ZZPhase, Unitary1q, Unitary2q
    assert all(c.mats is circuits[0].mats for c in circuits)  # one shared table
    proxy = np.array([H.queue_proxy(c) for c in circuits])
    assert np.diff(np.sort(proxy)).min() > 1e-9  # distinct beyond the rounding of a sum of sines: the queue order is known
    _assert_turns(info, len(circuits), 256, 4, cus, "vocabulary, shared table")
    assert info["threads"] == 256 and info["slots"] == 4 * cus == slots  # the four-workgroup shape, qk_build_kernel<4, false>
    assert not info["dropped"]
    host = H.host_states(circuits)
    later = H.later_turn_states(circuits, slots)
    assert max(host[i].max_bond() for i in later) >= 24  # a 48-column theta, factorised from L2 in this shape
    _assert_host(dev, host, "vocabulary")
    with _pinned(None):
        chunked, _ = _build_in_chunks(gpu_ctx, circuits, slots, 256, max_bond=32)
    _assert_same(dev, chunked, cases("four").reproducible, "vocabulary, against first-turn builds")


def test_shared_and_per_state_tables_agree_on_later_turn_states(gpu_ctx, cases, vocabulary):
    """The 40 later-turn states and 24 others: one shared matrix table (stride 0) and the same table repeated per state (stride
    n_mats) give the same bits, and -- on a builder that repeats itself -- the bits those states have in the build beyond the slots."""
    from qml_cutensornet_amd.engine import _GateProgram

    circuits, dev, _, slots = vocabulary
    later = sorted(H.later_turn_states(circuits, slots).tolist())
    pick = later + [i for i in range(len(circuits)) if i not in later][:24]
    assert len(pick) == 64 == len(set(pick))
    some = [circuits[i] for i in pick]
    with _pinned(None):
        shared = _GateProgram("test", some)
        assert shared.stride == 0 and shared.n_mats >= 10
        dims_a, a = _download(shared.build(gpu_ctx, 1 - 1e-16, 1e-16, 32, 0), len(some), 10)
        per_state = _GateProgram("test", some)
        per_state.mats, per_state.stride = np.ascontiguousarray(np.stack([shared.mats] * len(some))), shared.n_mats
        dims_b, b = _download(per_state.build(gpu_ctx, 1 - 1e-16, 1e-16, 32, 0), len(some), 10)
    assert np.array_equal(dims_a, dims_b)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for k, i in enumerate(pick):
        assert np.array_equal(dims_b[k], dev[i].bond_dims())
        if cases("four").reproducible:
            assert np.array_equal(b[k], np.concatenate([t.reshape(-1) for t in dev[i].tensors])), f"state {i}"


# ---- 3. trajectories
TRAJECTORY_LAYERS = 4  # bonds reach 16 at n = 8


def trajectory_gates(n, x):
    """Codes 10 and 11, drawn and forced: four layers of the noisy brickwork of tests/test_channels_host.py (AmplitudeDamping behind
    every two-qubit gate, a Measure), a forced Project and a forced Project2q of generic matrices, and four layers of the one of
    tests/test_channels2_host.py (Depolarizing2q behind every two-qubit gate, a Measure2q)."""
    rng = np.random.default_rng(77)
    m1 = np.eye(2) + 0.3 * (rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2)))
    m2 = np.eye(4) + 0.2 * (rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4)))
    return (noisy_brickwork(n, TRAJECTORY_LAYERS, x, seed=5) + [("Project", [2], [m1]), ("Project2q", [n - 2, n - 3], [m2])]
            + noisy2_brickwork(n, TRAJECTORY_LAYERS, x, seed=6))


def trajectory_program(n_states, n=8):
    """(circuits, state_index, trajectory): distinct names for every state.  Only the angles of the Rz / Ry data rotations depend on
    the data point, so the first circuit is bound from its gate list and the others take its program with their own angles (the
    last one is checked against its own gate list)."""
    X = features(n_states, n, 41)
    c0 = from_gates(n, trajectory_gates(n, X[0]))
    rot = np.isin(c0.op, (1, 5))

    def bind(x):
        alpha = c0.alpha.copy()
        alpha[rot] = x[c0.q0[rot]]
        return dataclasses.replace(c0, alpha=alpha)

    circuits = [c0] + [bind(x) for x in X[1:]]
    last = from_gates(n, trajectory_gates(n, X[-1]))
    for f in dataclasses.fields(last):
        assert np.array_equal(getattr(last, f.name), getattr(circuits[-1], f.name)), f.name
    s = np.arange(n_states)
    return circuits, (3 + 2 * s).astype(np.uint32), ((5 * s) % 11).astype(np.uint32)


@pytest.mark.parametrize("wgs,threads,per_cu", [("1", 512, 1), (None, 256, 4)])
def test_trajectories_do_not_depend_on_the_turn(gpu_ctx, cus, wgs, threads, per_cu):
    """<MINWG, true>: pinned to 512 threads, and the four-workgroup shape a program of trajectories takes on its own at max_bond <= 32."""
    import qml_cutensornet_amd as Q

    with _pinned(wgs):
        probe_c, si, tr = trajectory_program(2)
        _, probe = gpu_ctx.build_mps(probe_c, max_bond=32, seed=SEED, state_index=si, trajectory=tr)
        assert probe["threads"] == threads and probe["slots"] == per_cu * cus
        slots = probe["slots"]
        circuits, si, tr = trajectory_program(slots + H.BUILDER_TURN_EXTRA)
        c0 = circuits[0]
        # no XXPhase, YYPhase or ZZPhase gate: every proxy is an empty sum, exactly 0 on the host too, and the queue is the input order
        assert {10, 11} <= set(np.asarray(c0.op).tolist()) and not np.isin(np.asarray(c0.op), (2, 6, 7)).any() and {H.queue_proxy(c) for c in circuits} == {0.0}
        kw = dict(max_bond=32, seed=SEED, state_index=si, trajectory=tr)
        dev, info = gpu_ctx.build_mps(circuits, **kw)
        _assert_turns(info, len(circuits), threads, per_cu, cus, f"trajectories, {threads} threads")
        assert info["threads"] == threads and info["slots"] == per_cu * cus  # (None, 256, 4): 4 x CUs, qk_build_kernel<4, true>
        assert info["branches"].shape == (len(circuits), c0.n_channel_gates) and info["branches"].min() >= 0
        assert len({tuple(m.branches.tolist()) for m in dev}) > len(dev) // 2  # the trajectories differ
        chunked, _ = _build_in_chunks(gpu_ctx, circuits, slots, threads, **kw)
        for k, (a, b) in enumerate(zip(dev, chunked)):  # tensors, logw, branches and fidelity: bit for bit, unconditionally
            assert _same_bits(a, b), f"state {k} (queue position {k}) differs from its first-turn build"
            assert info["logw"][k] == a.logw and np.array_equal(info["branches"][k], a.branches)
        later = list(range(slots, len(circuits)))
        for k in later[::5]:  # 8 of the later-turn states built alone
            alone, _ = gpu_ctx.build_mps([circuits[k]], max_bond=32, seed=SEED, state_index=int(si[k]), trajectory=int(tr[k]))
            assert _same_bits(alone[0], dev[k]), f"state {k} built alone"
        assert len(later[::5]) == 8
    margin, hosts = np.inf, []
    for k in later[:24]:
        m, mg = Q.simulate(circuits[k], 1 - 1e-16, seed=SEED, state_index=int(si[k]), trajectory=int(tr[k]), margin=True)
        hosts.append(m)
        margin = min(margin, mg)
    assert margin >= 1e-6  # the condition of the comparison
    for k, mh in zip(later[:24], hosts):
        md = dev[k]
        assert np.array_equal(md.branches, mh.branches) and np.array_equal(md.bond_dims(), mh.bond_dims()), f"state {k}"
        assert abs(abs(R.mps_inner(md.tensors, mh.tensors)) ** 2 - 1) < 1e-10, f"state {k}"
        assert abs(md.logw - mh.logw) < 1e-10 and abs(md.fidelity - 1.0) < 1e-12, f"state {k}"


# ---- 4. partial builds
@pytest.mark.parametrize("order", ["default", "ascending"])
def test_partial_build_beyond_the_slots(gpu_ctx, cus, order):
    """A dropped state stops its workgroup at the offending gate; the next state of that workgroup is an ordinary one (default
    order: the droppers come first), or the other way round (ascending order)."""
    name, wgs, per_cu, threads, cap, least = H.BUILDER_TURN_PARTIAL
    with _pinned(wgs, ordered=order == "default"):
        _, probe = gpu_ctx.build_mps(H.builder_turn_circuits(name, 0, 2), max_bond=cap, partial=True)
        slots = probe["slots"]
        circuits = H.builder_turn_circuits(name, slots)
        host = H.host_states(circuits)  # uncapped
        perm = np.arange(len(circuits)) if order == "default" else H.ascending_by_proxy(circuits)
        circuits, host = [circuits[i] for i in perm], [host[i] for i in perm]
        dev, info = gpu_ctx.build_mps(circuits, max_bond=cap, partial=True)  # (no error is raised)
        _assert_turns(info, len(circuits), threads, per_cu, cus, f"partial build at cap {cap}, {order} order")
        chunked, dropped_b = _build_in_chunks(gpu_ctx, circuits, slots, threads, max_bond=cap, partial=True)
        one, _ = gpu_ctx.build_mps(circuits[:slots // 2], max_bond=cap, partial=True)
    reproducible = all((a is None and b is None) or (a is not None and b is not None and _same_bits(a, b)) for a, b in zip(one, chunked))
    above = np.array([m.max_bond() > cap for m in host])
    later = H.later_turn_states(circuits, slots, ordered=order == "default")
    first = np.setdiff1d(np.arange(len(circuits)), later)
    dropped = np.zeros(len(circuits), dtype=bool)
    dropped[info["dropped"]] = True
    print(f"partial, {order} order: {int(dropped.sum())} dropped, {int(dropped[later].sum())} of them among the {len(later)} later-turn states; first-turn builds repeat: {reproducible}")
    # what the device did, not what the host's final bonds predict (a state is dropped when a bond outgrows the cap at any gate)
    assert dropped[later].sum() >= least and dropped[first].sum() >= least
    if order == "default":  # ordinary states follow droppers on the same workgroups, and droppers follow droppers
        assert (~dropped[later]).sum() >= least
    else:  # the other way round: ordinary states among the first, the heaviest states -- droppers mostly -- after them
        assert (~dropped[first]).sum() >= least
    assert sorted(info["dropped"]) == sorted(dropped_b)
    assert set(np.flatnonzero(above).tolist()) <= set(info["dropped"])  # (a transient bond may exceed the cap even if the final ones do not)
    _assert_same(dev, chunked, reproducible, f"partial, {order} order, against first-turn builds")
    for k, m in enumerate(dev):
        assert (m is None) == bool(dropped[k])
        if m is not None:
            assert m.max_bond() <= cap and abs(abs(R.mps_inner(m.tensors, host[k].tensors)) ** 2 - 1) < 1e-10, f"survivor {k}"


# ---- 5. snapshots and resume
def _assert_scan_equal(scan, ref_states, ref_infos, reproducible, what):
    for j in range(len(scan)):
        _assert_same(scan.states(j), ref_states[j], reproducible, f"{what}, snapshot {j}")
        got = scan.info(j)
        assert np.array_equal(got["centre"], ref_infos[j]["centre"]), f"{what}, snapshot {j}: centres"
        assert np.array_equal(got["dims"], ref_infos[j]["dims"])


def _scan_in_chunks(ctx, circuits, cps, slots, threads, **kw):
    """reference (b) of a scan: per snapshot the states and {"centre", "dims", "logw"} of first-turn scans"""
    states, infos = [[] for _ in cps], [[] for _ in cps]
    for r in _chunks(len(circuits), slots):
        cut = {k: (v[r.start:r.stop] if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
        with ctx.build_mps_scan([circuits[i] for i in r], cps, **cut) as part:
            _assert_first_turn(part.launch, len(r), threads)
            for j in range(len(cps)):
                states[j] += part.states(j)
                infos[j].append(part.info(j))
    return states, [{k: np.concatenate([i[k] for i in per]) for k in ("centre", "dims", "logw")} for per in infos]


def test_snapshots_and_resume_beyond_the_slots(gpu_ctx, cases):
    case = cases("two")
    import qml_cutensornet_amd as Q

    ends = Q.KernelStateAnsatz(case.n, case.reps, 1.0, Q.entanglement_graph(case.n, case.d)).layer_ends()
    assert len(ends) == 3
    plain, _ = case.big()
    with _pinned(case.wgs):
        ref_states, ref_infos = _scan_in_chunks(gpu_ctx, case.circuits, ends, case.slots, case.threads, max_bond=case.max_bond)
        with gpu_ctx.build_mps_scan(case.circuits, ends, max_bond=case.max_bond) as scan:
            _assert_turns({**scan.launch, "kernel_ms": scan.kernel_ms}, len(case.circuits), case.threads, case.per_cu, case.cus, "scan of 'two', three checkpoints")
            assert scan.info(0)["grid"] == scan.launch["grid"]
            _assert_scan_equal(scan, ref_states, ref_infos, case.reproducible, "scan")
            final = scan.states(2)
            _assert_same(final, plain, case.reproducible, "last snapshot against the plain build")
            rest = [c.sliced(ends[1], ends[2]) for c in case.circuits]
            with gpu_ctx.build_mps_scan(rest, [ends[2] - ends[1]], initial=(scan, 1), max_bond=case.max_bond) as resumed:  # wg_load_snapshot into a re-used arena
                _assert_turns({**resumed.launch, "kernel_ms": resumed.kernel_ms}, len(rest), case.threads, case.per_cu, case.cus, "resumed from the middle snapshot")
                _assert_same(resumed.states(0), final, case.reproducible, "resumed from the middle snapshot")
                assert np.array_equal(resumed.info(0)["centre"], scan.info(2)["centre"])


def test_snapshots_and_resume_of_trajectories_beyond_the_slots(gpu_ctx, cus):
    """The same with a channel program in the 512-thread shape: the log-weight travels with the snapshot.  Bit for bit."""
    with _pinned("1"):
        probe_c, si, tr = trajectory_program(2)
        _, probe = gpu_ctx.build_mps(probe_c, max_bond=32, seed=SEED, state_index=si, trajectory=tr)
        slots = probe["slots"]
        circuits, si, tr = trajectory_program(slots + H.BUILDER_TURN_EXTRA)
        c0 = circuits[0]
        at = np.flatnonzero((np.asarray(c0.op) == 10) | (np.asarray(c0.op) == 11))
        cps = [int(at[len(at) // 3]) + 1, int(at[2 * len(at) // 3]), c0.n_gates]  # behind a channel gate, in front of one, the whole program
        kw = dict(max_bond=32, seed=SEED, state_index=si, trajectory=tr)
        ref_states, ref_infos = _scan_in_chunks(gpu_ctx, circuits, cps, slots, 512, **kw)
        with gpu_ctx.build_mps_scan(circuits, cps, **kw) as scan:
            _assert_turns({**scan.launch, "kernel_ms": scan.kernel_ms}, len(circuits), 512, 1, cus, "scan of trajectories, three checkpoints")
            _assert_scan_equal(scan, ref_states, ref_infos, True, "scan of trajectories")
            for j in range(3):
                assert np.array_equal(scan.info(j)["logw"], ref_infos[j]["logw"]) and np.array_equal(scan.info(j)["logw"], [m.logw for m in scan.states(j)])
            assert np.all(scan.info(0)["logw"] != scan.info(2)["logw"])
            final, done = scan.states(2), int(np.count_nonzero(at < cps[1]))
            rest = [c.sliced(cps[1], c.n_gates) for c in circuits]
            with gpu_ctx.build_mps_scan(rest, [c0.n_gates - cps[1]], initial=(scan, 1), **kw) as resumed:
                _assert_turns({**resumed.launch, "kernel_ms": resumed.kernel_ms}, len(rest), 512, 1, cus, "trajectories resumed from the middle snapshot")
                for k, (a, b) in enumerate(zip(resumed.states(0), final)):
                    assert a.fidelity == b.fidelity and a.logw == b.logw and np.array_equal(a.branches, b.branches[done:]), f"state {k}"
                    assert all(np.array_equal(x, y) for x, y in zip(a.tensors, b.tensors)), f"state {k}"


# ---- 6. build_mps_set beyond the slots
def test_built_set_beyond_the_slots(gpu_ctx, cases):
    case = cases("four")
    states, _ = case.big()
    with _pinned(case.wgs):
        dset, info = gpu_ctx.build_mps_set(case.circuits, max_bond=case.max_bond)
    _assert_turns(info, len(case.circuits), case.threads, case.per_cu, case.cus, "build_mps_set of 'four'")
    assert np.array_equal(info["dims"], np.array([m.bond_dims() for m in states]))
    K = gpu_ctx.gram(dset)
    with gpu_ctx.upload(states) as up:
        assert np.abs(K - gpu_ctx.gram(up)).max() < 1e-12
    dset.close()
    later = H.later_turn_states(case.circuits, case.slots)
    K_ref = R.gram_from_mps([m.tensors for m in case.host], [case.host[i].tensors for i in later])  # rows: the 40 later-turn states
    assert np.abs(K[later] - K_ref).max() < 1e-9
