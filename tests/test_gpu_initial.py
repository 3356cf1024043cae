"""GPU tests of building from given states (``qk_built_from_set``, ``Context.seed``, ``initial=`` of the build calls and
``initial_states=`` of the drivers): the verbatim path downloads the bits of an uninterrupted scan in every launch shape and the bits
of the set it was made from on bonds 1 .. 33; the sweep path against ``mps.seed_state`` and ``simulate(initial=)`` on 14-site
general-gauge, unnormalised states on either side of the 48-column switch to the matrix-core Jacobi, one of them rank deficient;
``index`` (broadcast, trajectories) and workgroups that build more than one state, bit for bit; the rejections; and the drivers.

Tolerances: what the issue of this feature sets -- seed against input: overlap >= 1 - 1e-12, isometry residual <= 1e-12, norms to
1e-12 relative; device against host builder as everywhere in this suite: bonds and branches equal, |<dev|host>|^2 >= 1 - 1e-10,
log-weights to 1e-10, Gram entries and driver matrices to 1e-9.  Device and host draw the same branches when no draw of the host
sits within 1e-6 of a threshold: asserted first.  The rank-deficient state takes ``value_of_zero=1e-12`` as in
tests/test_gpu_compress.py: a gauge of cond <= 4 leaves rounding of about 1e-15 of the norm in the directions a bond does not need."""
import ctypes as C

import numpy as np
import pytest

from helpers import capped_mps, scrambled
from oracle import restatement as R
from test_feature_map_host import zz_template
from test_gpu_channels import _bloch, same_bits
from test_gpu_conditions import pooling_ansatz
from test_gpu_matrix_gates import circuits_12
from test_initial_host import left_residual
from test_matrix_gates_host import features, from_gates, mps_vector

pytestmark = pytest.mark.gpu

SEED = 31


def same_tensors(a, b):
    return len(a.tensors) == len(b.tensors) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a.tensors, b.tensors))


def general_states(n, chi, count, seed, scales=(3.7, 0.3, 1.0)):
    """``count`` random chains on the bonds min(2^k, 2^(n-k), chi) in a dense complex gauge, unnormalised."""
    rng = np.random.default_rng(seed)
    return [scrambled(capped_mps(n, chi, rng), rng, scale=scales[k % len(scales)]) for k in range(count)]


# ---- 1. the verbatim path is exact
@pytest.mark.parametrize("shape", ["512 threads", "two workgroups", "four workgroups, capped at 32"])
def test_verbatim_seed_resumes_with_the_bits_of_the_uninterrupted_scan(gpu_ctx, monkeypatch, shape):
    """A verbatim seed starts at fidelity 1, so the resumed build multiplies the factors of its own gates only: its fidelity is the
    uninterrupted run's bit for bit where the snapshot's own fidelity is exactly 1.  That holds at the early cut (inside layer 2;
    the five layers behind it reach bond 64 in every launch shape) and is asserted there; at the late cut (inside layer 4, bonds up
    to 16 in the seed) the snapshot has lost an ulp or two in two of the three states, so there the tensors and the bonds are
    compared bit for bit and the fidelity as a product."""
    wgs, kw, threads = {"512 threads": ("1", {}, 512), "two workgroups": ("2", {}, 256), "four workgroups, capped at 32": ("4", dict(max_bond=32, truncate=True), 256)}[shape]
    monkeypatch.setenv("QK_BUILD_WGS", wgs)
    circuits = circuits_12()
    c0 = circuits[0]
    n_gates = c0.n_gates
    two_q = np.flatnonzero(c0.op == 9)
    early, late = int(two_q[9]) + 1, int(two_q[19]) + 3
    with gpu_ctx.build_mps_scan(circuits, [early, late, n_gates], **kw) as scan:
        assert scan.launch["threads"] == threads
        want = scan.states(-1)
        assert max(m.max_bond() for m in want) == (32 if kw else 64)
        for j, cut in enumerate((early, late)):
            info0 = scan.info(j)
            tail = [c.sliced(cut, n_gates) for c in circuits]
            with scan.set(j) as s0:
                assert s0.centre >= 0 and np.all(info0["centre"] == s0.centre)
                with gpu_ctx.seed(s0) as seed:
                    si = seed.info(0)
                    assert seed.checkpoints == [0] and len(seed) == 1
                    assert np.array_equal(si["dims"], info0["dims"]) and np.array_equal(si["centre"], info0["centre"])
                    assert np.all(si["fidelity"] == 1.0) and np.all(si["logw"] == 0.0) and np.all(si["norm"] == 1.0) and si["branches"].shape == (3, 0)
                    assert (si["grid"], si["threads"], si["slots"]) == (0, 0, 0)  # nothing was factorised
                    for a, b in zip(seed.states(0), scan.states(j)):
                        assert same_tensors(a, b)
                    with gpu_ctx.build_mps_scan(tail, [n_gates - cut], initial=(seed, 0), **kw) as resumed:
                        assert resumed.launch["threads"] == threads
                        got = resumed.states(-1)
                with gpu_ctx.build_mps_scan(tail, [n_gates - cut], initial=s0, **kw) as direct:  # the same through initial= with the set itself
                    again = direct.states(-1)
            if cut == early:
                assert np.all(info0["fidelity"] == 1.0) and info0["dims"].max() == 4
            else:
                assert info0["dims"].max() == 16
            for a, b, c, f0 in zip(got, want, again, info0["fidelity"]):
                assert np.array_equal(a.bond_dims(), b.bond_dims()) and same_tensors(a, b)
                assert same_tensors(c, b) and c.fidelity == a.fidelity
                if cut == early:
                    assert a.fidelity == b.fidelity
                else:
                    assert abs(a.fidelity * f0 - b.fidelity) <= 4 * np.finfo(float).eps


# ---- 2. the unpack kernel on the bonds of the padding rules
UNPACK_CAPS = (3, 5, 17, 33)


def test_verbatim_seed_downloads_the_bits_of_its_set(gpu_ctx):
    circuits = circuits_12()
    bonds = set()
    for cap in UNPACK_CAPS:
        xs, info = gpu_ctx.build_mps_set(circuits, max_bond=cap, truncate=True)
        with xs:
            bonds |= set(int(d) for d in np.unique(info["dims"]))
            assert xs.centre >= 0
            own = xs.download()
            with gpu_ctx.seed(xs) as seed:
                assert np.array_equal(seed.info(0)["dims"], info["dims"])
                for a, b in zip(seed.states(0), own):
                    assert same_tensors(a, b)
            with gpu_ctx.seed(xs, index=[2, 0, 0, 1]) as seed:  # the tables repeat: a snapshot of four states
                assert seed.info(0)["heap_bytes"] == 16 * sum(own[k].nbytes() // 16 for k in (2, 0, 0, 1))
                for a, k in zip(seed.states(0), (2, 0, 0, 1)):
                    assert same_tensors(a, own[k])
    assert {1, 2, 3, 5, 16, 17, 33} <= bonds


# ---- 3. the sweep path
N_SWEEP = 14
ZERO = 1e-12


def sweep_inputs():
    """Four 14-site states: chi = 20 (factorised in LDS) and chi = 70 (the preconditioned block Jacobi on the matrix cores), and a
    chi = 20 state whose bonds are 3 wider than their ranks."""
    a, b = general_states(N_SWEEP, 20, 2, 201), general_states(N_SWEEP, 70, 2, 202)
    rng = np.random.default_rng(203)
    wide = scrambled(capped_mps(N_SWEEP, 20, rng), rng, scale=0.6, grow=3)
    return [a[0], b[0], wide, b[1], a[1]]


def sweep_gates(x):
    """Two entangling layers on 14 qubits with a Measure in between and an X and an XXPhase conditioned on it."""
    n = N_SWEEP
    gates = [("Ry", [q], [float(x[q])]) for q in range(n)] + [("XXPhase", [q, q + 1], [float(x[q]) * 0.5]) for q in range(0, n - 1, 2)]
    A = len(gates)
    gates += [("Measure", [6], []), ("X", [7], [], (A, 1)), ("XXPhase", [8, 9], [0.3], (A, 0))]
    gates += [("Rz", [q], [float(x[q])]) for q in range(n)] + [("ZZPhase", [q, q + 1], [float(x[q + 1]) * 0.5]) for q in range(1, n - 1, 2)]
    # the measurement leaves the bonds beside qubit 6 above their ranks; the device's centre moves reveal a rank, the host's QR does not:
    # a two-qubit gate on every bond behind it makes both builders cut there, and the bond tables comparable
    return gates + [("YYPhase", [q, q + 1], [float(x[q]) * 0.25]) for q in range(0, n - 1, 2)]


@pytest.fixture(scope="module")
def sweep_case(built):
    import qml_cutensornet_amd as Q
    from qml_cutensornet_amd import mps

    inputs = sweep_inputs()
    seeds = [mps.seed_state(m, ZERO) for m in inputs]
    circuits = [from_gates(N_SWEEP, sweep_gates(x)) for x in features(len(inputs), N_SWEEP, 91)]
    host, margin = [], np.inf
    for s, (c, (m, _)) in enumerate(zip(circuits, seeds)):
        h, mg = Q.simulate(c, 1 - 1e-16, seed=SEED, state_index=s, margin=True, initial=m, initial_centre=N_SWEEP - 1)
        host.append(h)
        margin = min(margin, mg)
    return inputs, seeds, circuits, host, margin


@pytest.mark.parametrize("chi", [20, 70])
def test_sweep_seed_is_canonical_and_the_input_state(gpu_ctx, sweep_case, chi):
    """The chi = 70 case is the one that needs the polish of ``qk_seed_gather_kernel``.  From 48 columns on the factorisation of
    ``qk_compress_kernel``, which the seed runs unchanged, is the preconditioned block Jacobi; it forms W = A V by a matrix product
    and the isometry as W / sigma, so a column loses orthogonality in proportion to sigma_max / sigma -- 1.8e6 at bond 8 of these
    states (``MPS.bond_spectra``), times the rounding of the product: 2.4e-9 and 7.0e-9 measured on the two chi = 70 states before
    the polish, 3.2e-13 to 8.2e-13 on the chi = 20 states (one-sided Jacobi in LDS).  With the polish (one Newton-Schulz step per
    site whose defect lies above 1e-13, the next site taking the inverse factor) every state measures 6.7e-14 to 8.1e-14, which is
    what a site below that threshold keeps; 1 - overlap stays at 6.8e-14 and the reported norm at 9.1e-14 relative."""
    inputs, seeds, *_ = sweep_case
    assert [m.max_bond() for m in inputs] == [20, 70, 23, 70, 20]
    with gpu_ctx.upload(inputs) as xs:
        assert xs.centre == -1
        with gpu_ctx.seed(xs, value_of_zero=ZERO) as seed:
            info, got = seed.info(0), seed.states(0)
            assert seed.checkpoints == [0] and info["threads"] == 256 and info["grid"] >= 1 and seed.kernel_ms > 0
    assert np.all(info["centre"] == N_SWEEP - 1) and np.all(info["logw"] == 0.0)
    mine = [k for k, m in enumerate(inputs) if (m.max_bond() == 70) == (chi == 70)]
    assert len(mine) == (2 if chi == 70 else 3)
    figures = []
    for k in mine:
        m, g, (ref, norm) = inputs[k], got[k], seeds[k]
        nn = R.mps_inner(m.tensors, m.tensors).real
        overlap = abs(R.mps_inner(g.tensors, m.tensors)) ** 2 / nn
        resid = max(left_residual(t) for t in g.tensors[:-1])
        gg = R.mps_inner(g.tensors, g.tensors).real
        print(f"sweep seed, state {k} (bond {m.max_bond()}): 1 - overlap = {1 - overlap:.3e}, isometry residual {resid:.3e}, norm - 1 = {gg - 1:.3e}, "
              f"norm rel. error {abs(info['norm'][k] - np.sqrt(nn)) / np.sqrt(nn):.3e}, fidelity - 1 = {info['fidelity'][k] - 1:.3e}")
        assert overlap >= 1 - 1e-12 and abs(gg - 1) <= 1e-12
        assert np.array_equal(g.bond_dims(), ref.bond_dims()) and np.array_equal(info["dims"][k], ref.bond_dims())
        assert abs(info["norm"][k] - np.sqrt(nn)) <= 1e-12 * np.sqrt(nn) and abs(info["norm"][k] - norm) <= 1e-12 * norm
        assert abs(info["fidelity"][k] - ref.fidelity) <= 1e-12 and g.fidelity == info["fidelity"][k]
        figures.append(resid)
    if chi == 20:
        assert got[2].max_bond() == 20 and inputs[2].max_bond() == 23  # the rank-deficient bonds shrank to their ranks
    assert max(figures) <= 1e-12, f"isometry residuals {figures}"


def test_build_on_sweep_seed_matches_the_host_builder(gpu_ctx, sweep_case):
    inputs, _, circuits, host, margin = sweep_case
    assert margin >= 1e-6  # the condition of the comparison
    ns = len(inputs)
    with gpu_ctx.upload(inputs) as xs, gpu_ctx.seed(xs, value_of_zero=ZERO) as seed:
        with gpu_ctx.build_mps_scan(circuits, [circuits[0].n_gates], initial=(seed, 0), seed=SEED, state_index=np.arange(ns)) as scan:
            dev, dset = scan.states(-1), scan.set(-1)
            print(f"two layers on the sweep seeds: kernel_ms = {scan.kernel_ms:.1f}, bonds up to {max(m.max_bond() for m in dev)}")
    with dset, gpu_ctx.upload(host) as hx:
        assert np.abs(gpu_ctx.gram(dset) - gpu_ctx.gram(hx)).max() < 1e-9
    assert {int(m.branches[0]) for m in host} == {0, 1}
    for k, (d, h) in enumerate(zip(dev, host)):
        print(f"state {k}: branches {d.branches.tolist()} / {h.branches.tolist()}, bonds equal {np.array_equal(d.bond_dims(), h.bond_dims())} (up to {d.max_bond()} / {h.max_bond()}), "
              f"1 - overlap = {1 - abs(R.mps_inner(d.tensors, h.tensors)) ** 2:.3e}, logw difference {d.logw - h.logw:.3e}, fidelity {d.fidelity:.15f} / {h.fidelity:.15f}")
    for d, h in zip(dev, host):
        assert np.array_equal(d.branches, h.branches) and np.array_equal(d.bond_dims(), h.bond_dims())
        assert abs(R.mps_inner(d.tensors, h.tensors)) ** 2 >= 1 - 1e-10 and abs(d.logw - h.logw) <= 1e-10
        assert abs(d.fidelity - h.fidelity) < 1e-9 * max(1.0, h.fidelity)


# ---- 4. index: broadcast and trajectories
def traj_gates(x, n=8):
    gates = [("Ry", [q], [float(x[q])]) for q in range(n)] + [("XXPhase", [q, q + 1], [float(x[q])]) for q in range(0, n - 1, 2)]
    A = len(gates)
    gates += [("Measure", [3], []), ("X", [4], [], (A, 1)), ("Depolarizing2q", [5, 6], [0.3]), ("AmplitudeDamping", [1], [0.2])]
    return gates + [("YYPhase", [q, q + 1], [float(x[q + 1])]) for q in range(1, n - 1, 2)]


def test_broadcast_and_trajectories_through_index_are_bit_stable(gpu_ctx):
    import qml_cutensornet_amd as Q

    n = 8
    inputs = general_states(n, 4, 3, 301)
    X = features(5, n, 302)
    # one state under five circuits
    five = [from_gates(n, traj_gates(x)) for x in X]
    kw = dict(seed=SEED, state_index=np.arange(5), trajectory=np.zeros(5, dtype=np.int64))
    all5, _ = gpu_ctx.build_mps(five, initial=inputs[1], **kw)
    again, _ = gpu_ctx.build_mps(five, initial=inputs[1], **kw)
    assert len({tuple(m.branches.tolist()) for m in all5}) > 1
    for k, (a, b) in enumerate(zip(all5, again)):
        alone, _ = gpu_ctx.build_mps([five[k]], seed=SEED, state_index=k, trajectory=0, initial=inputs[1])
        assert same_bits(a, b) and same_bits(a, alone[0])
    # three input states x three trajectories
    T = 3
    index = np.repeat(np.arange(3), T)
    traj = np.tile(np.arange(T), 3)
    nine = [five[s] for s in index]
    ref, info = gpu_ctx.build_mps(nine, seed=SEED, state_index=index, trajectory=traj, initial=inputs, initial_index=index)
    assert len({tuple(r) for r in info["branches"].tolist()}) > 3
    rerun, _ = gpu_ctx.build_mps(nine, seed=SEED, state_index=index, trajectory=traj, initial=inputs, initial_index=index)
    order = np.array([7, 2, 4, 0, 8, 3, 6, 1, 5])
    shuffled, _ = gpu_ctx.build_mps([nine[k] for k in order], seed=SEED, state_index=index[order], trajectory=traj[order], initial=inputs, initial_index=index[order])
    with gpu_ctx.seed(inputs, index=index) as seed:  # an explicit seed, used twice
        assert seed.n_states == 9 and np.array_equal(seed.info(0)["norm"][::T], seed.info(0)["norm"][1::T])
        seeded, _ = gpu_ctx.build_mps(nine, seed=SEED, state_index=index, trajectory=traj, initial=(seed, 0))
    for k in range(9):
        alone, _ = gpu_ctx.build_mps([nine[k]], seed=SEED, state_index=int(index[k]), trajectory=int(traj[k]), initial=[inputs[index[k]]])
        assert same_bits(ref[k], rerun[k]) and same_bits(ref[k], alone[0]) and same_bits(ref[k], seeded[k]), f"build state {k}"
        assert same_bits(ref[order[k]], shuffled[k]), f"build state {order[k]} at position {k}"
    # and against the host builder
    for k in (0, 4, 8):
        h, margin = Q.simulate(nine[k], 1 - 1e-16, seed=SEED, state_index=int(index[k]), trajectory=int(traj[k]), margin=True, initial=inputs[index[k]])
        assert margin >= 1e-6
        assert np.array_equal(h.branches, ref[k].branches) and abs(h.logw - ref[k].logw) <= 1e-10 and abs(R.mps_inner(h.tensors, ref[k].tensors)) ** 2 >= 1 - 1e-10


# ---- 5. workgroups that build more than one state
def test_later_turn_states_from_a_seed_are_the_bits_of_first_turn_states(gpu_ctx, monkeypatch):
    monkeypatch.setenv("QK_BUILD_WGS", "4")
    n = 6
    inputs = general_states(n, 4, 3, 401)
    X = features(4, n, 402)
    base = [from_gates(n, [("Ry", [q], [float(x[q])]) for q in range(n)] + [("XXPhase", [q, q + 1], [float(x[q])]) for q in range(0, n - 1, 2)]
                       + [("Rz", [q], [float(x[q])]) for q in range(n)] + [("ZZPhase", [q, q + 1], [float(x[q + 1])]) for q in range(1, n - 1, 2)]) for x in X]
    kw = dict(max_bond=8)
    _, probe = gpu_ctx.build_mps(base, initial=inputs[0], **kw)
    slots = probe["slots"]
    assert probe["threads"] == 256 and probe["grid"] == 4 < slots
    n_states = slots + 8
    circuits = [base[k % 4] for k in range(n_states)]
    index = (np.arange(n_states) % 3).astype(np.int32)
    dev, info = gpu_ctx.build_mps(circuits, initial=inputs, initial_index=index, **kw)
    print(f"turns from a seed: {n_states} states on a grid of {info['grid']} x {info['threads']} threads ({info['slots']} slots), kernel_ms = {info['kernel_ms']:.1f}")
    assert info["threads"] == 256 and info["grid"] == info["slots"] == slots < n_states
    size = slots // 2
    for s0 in range(0, n_states, size):  # every state again as the first of its workgroup
        part, pinfo = gpu_ctx.build_mps(circuits[s0:s0 + size], initial=inputs, initial_index=index[s0:s0 + size], **kw)
        assert pinfo["grid"] == len(part) <= slots // 2
        for k, (a, b) in enumerate(zip(part, dev[s0:s0 + size])):
            assert same_bits(a, b), f"state {s0 + k}"
    assert len({m.tensors[2].tobytes() for m in dev[:12]}) == 12  # twelve (circuit, input) pairs: none is another's copy


# ---- 6. rejections
def test_rejections_by_name(gpu_ctx):
    from qml_cutensornet_amd import engine
    from qml_cutensornet_amd.engine import QkError

    n = 6
    inputs = general_states(n, 4, 3, 501)
    c = from_gates(n, [("Ry", [q], [0.3]) for q in range(n)] + [("XXPhase", [2, 3], [0.4])])
    with gpu_ctx.upload(inputs) as xs:
        with xs.to_f32() as x32, pytest.raises(QkError, match="complex64"):
            gpu_ctx.seed(x32)
        other = engine.Context(0)
        try:
            with pytest.raises(QkError, match="another context"):
                other.seed(xs)
        finally:
            other.close()
        for bad in ([0, 3], [-1]):
            with pytest.raises(QkError, match="outside the set"):
                gpu_ctx.seed(xs, index=bad)
        with pytest.raises(ValueError, match="index"):
            gpu_ctx.seed(xs, index=[])
        for zero in (-1.0, float("nan"), float("inf")):
            with pytest.raises(QkError, match="value_of_zero"):
                gpu_ctx.seed(xs, value_of_zero=zero)
        L, h = engine.lib(), C.c_void_p()
        idx = np.zeros(1, dtype=np.int32)
        for args, text in (((None, xs.handle, 3, None, 1e-16, 0, C.byref(h), None, None), "ctx is null"), ((gpu_ctx.handle, None, 3, None, 1e-16, 0, C.byref(h), None, None), "set is null"),
                           ((gpu_ctx.handle, xs.handle, 3, None, 1e-16, 0, None, None, None), "out is null"), ((gpu_ctx.handle, xs.handle, 0, idx.ctypes.data, 1e-16, 0, C.byref(h), None, None), "n_states"),
                           ((gpu_ctx.handle, xs.handle, 2, None, 1e-16, 0, C.byref(h), None, None), "n_states must be the set's"),
                           ((gpu_ctx.handle, xs.handle, 3, None, 1e-16, 2, C.byref(h), None, None), "unknown flags")):
            assert L.qk_built_from_set(*args) == -1 and text in L.qk_last_error().decode()  # QK_EINVAL
        with gpu_ctx.seed(xs) as seed, pytest.raises(QkError, match="beyond max_bond = 2"):
            gpu_ctx.build_mps([c] * 3, max_bond=2, initial=(seed, 0))
        with pytest.raises(ValueError, match="start 3 builds, the call has 2 circuits"):
            gpu_ctx.build_mps([c] * 2, initial=xs)
        with pytest.raises(ValueError, match="initial must be"):
            gpu_ctx.build_mps([c] * 3, initial="psi")
        with gpu_ctx.seed(xs) as seed:
            clean = seed.states(0)
    zero = inputs[1].copy()
    zero.tensors[2] = np.zeros_like(zero.tensors[2])
    with pytest.raises(QkError, match="state 1 has norm 0") as exc:
        gpu_ctx.seed([inputs[0], zero, inputs[2]])
    assert "qk_built_from_set" in str(exc.value)
    nan = inputs[2].copy()
    nan.tensors[4][1, 1, 0] = complex(0.0, float("nan"))
    with pytest.raises(QkError, match="state 2 holds an element that is not finite"):
        gpu_ctx.seed([inputs[0], inputs[1], nan, inputs[2]])
    with gpu_ctx.seed(inputs) as seed:  # the failed calls left nothing behind: the clean states come out as before
        for a, b in zip(seed.states(0), clean):
            assert same_bits(a, b)


# ---- 7. the drivers
@pytest.fixture(scope="module")
def driver_case(built):
    """8 qubits, 6 data points with one bond-4 input state each; the pooling ansatz (measurements, conditional unitaries) for the
    noisy driver and its feature map alone -- the same gates in front of the measurements -- for ``build_projected_kernel_matrix``,
    which takes no channels.  The reference features come from the host builder's dense vectors."""
    import qml_cutensornet_amd as Q

    n, T, seed = 8, 2, 8
    pooling, feature_map = pooling_ansatz(n), Q.CircuitAnsatz(n, list(zz_template(n, 2, 0.8, 2)))
    X = R.synthetic_features(6, n, 13)
    inputs = general_states(n, 4, 6, 601)
    margin, rows = np.inf, []
    for p, (x, m) in enumerate(zip(X, inputs)):
        row = []
        for t in range(T):
            h, mg = Q.simulate(pooling.circuit_for_data(x), 1 - 1e-16, seed=seed, state_index=p, trajectory=t, margin=True, initial=m)
            margin = min(margin, mg)
            row.append(_bloch(mps_vector(h), n))
        rows.append(np.mean(row, axis=0))
    noisy = np.array(rows)
    exact = np.array([_bloch(mps_vector(Q.simulate(feature_map.circuit_for_data(x), 1 - 1e-16, initial=m)), n) for x, m in zip(X, inputs)])
    want = lambda f: np.exp(-0.5 / n * ((f[:, None] - f[None, :]) ** 2).sum(axis=(2, 3)))  # noqa: E731
    return n, T, seed, pooling, feature_map, X, inputs, margin, want(exact), want(noisy)


@pytest.mark.parametrize("builder", ["device", "host"])
def test_drivers_from_given_states(driver_case, monkeypatch, builder):
    import qml_cutensornet_amd as Q
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_kernel_matrix, build_noisy_projected_kernel_matrix, build_projected_kernel_matrix

    monkeypatch.setenv("QK_BUILDER", builder)
    n, T, seed, pooling, feature_map, X, inputs, margin, want_exact, want_noisy = driver_case
    assert margin >= 1e-6  # device and host draw the same branches
    K = build_projected_kernel_matrix(SingleComm(), feature_map, X, truncation_error=1e-16, initial_states=inputs)
    assert K.shape == (6, 6) and np.abs(K - want_exact).max() < 1e-9
    Kxy = build_projected_kernel_matrix(SingleComm(), feature_map, X, Y=X[:4], truncation_error=1e-16, initial_states=inputs, initial_states_Y=inputs[:4])
    assert Kxy.shape == (4, 6) and np.abs(Kxy - want_exact[:4]).max() < 1e-9
    with pytest.raises(ValueError, match="trajectories"):  # the driver without trajectories refuses the measurements, with or without given states
        build_projected_kernel_matrix(SingleComm(), pooling, X, truncation_error=1e-16, initial_states=inputs)
    Kn = build_noisy_projected_kernel_matrix(SingleComm(), pooling, X, trajectories=T, noise_seed=seed, truncation_error=1e-16, initial_states=inputs)
    assert Kn.shape == (6, 6) and np.abs(Kn - want_noisy).max() < 1e-9
    assert np.abs(Kn - want_exact).max() > 1e-3 and np.abs(K - np.eye(6)).max() > 1e-3  # the measurements and the inputs matter
    # the fidelity kernel from given states, against the host builder's vectors
    vs = [mps_vector(Q.simulate(feature_map.circuit_for_data(x), 1 - 1e-16, initial=m)) for x, m in zip(X, inputs)]
    F = build_kernel_matrix(SingleComm(), feature_map, X, truncation_error=1e-16, initial_states=inputs)
    assert np.abs(F - np.array([[abs(np.vdot(p, q)) ** 2 for p in vs] for q in vs])).max() < 1e-9
    # |0...0> given as a state is the call without it
    zero = Q.MPS([np.array([1.0, 0.0], dtype=np.complex128).reshape(1, 2, 1) for _ in range(n)])
    for given in (zero, [zero] * 6):
        assert np.abs(build_projected_kernel_matrix(SingleComm(), feature_map, X, truncation_error=1e-16, initial_states=given)
                      - build_projected_kernel_matrix(SingleComm(), feature_map, X, truncation_error=1e-16)).max() < 1e-9
    assert np.abs(build_noisy_projected_kernel_matrix(SingleComm(), pooling, X, trajectories=T, noise_seed=seed, truncation_error=1e-16, initial_states=zero)
                  - build_noisy_projected_kernel_matrix(SingleComm(), pooling, X, trajectories=T, noise_seed=seed, truncation_error=1e-16)).max() < 1e-9
    with pytest.raises(ValueError, match="one per data point"):
        build_projected_kernel_matrix(SingleComm(), feature_map, X, truncation_error=1e-16, initial_states=inputs[:5])
