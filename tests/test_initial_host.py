"""Building from given states on the host (no GPU): ``mps.seed_state`` and ``initial=`` / ``initial_centre=`` of ``simulate``, the
numpy loop and the native builder (``qkb_simulate_initial``) against the dense state vector written out here -- 7 qubits, inputs in
a general gauge, unnormalised, with one bond of dimension 8 that has rank 3, under a program with rotations, a ``Unitary2q``, a
``Measure`` with a conditional ``X`` and a ``Depolarizing2q`` --, the split identity, the bit-for-bit resume from a checkpoint
snapshot, and the rejections.  The inputs and the program of this file are shared with tests/test_initial_san.py."""
import ctypes as C
import math

import numpy as np
import pytest

from helpers import scrambled
from test_channels2_host import _matrices
from test_channels_host import BUILDERS
from test_matrix_gates_host import apply_dense, from_gates, haar, mps_vector

N = 7
SEED = 77
RANK_BOND, RANK = 3, 3  # bond 3 (between sites 2 and 3) has dimension 8 and rank 3
MEASURE = 10  # list position of the Measure gate


def input_states(count=3):
    """General-gauge, unnormalised 7-site states on the bonds [1, 2, 4, 8, 8, 4, 2, 1]; bond 3 has rank 3."""
    import qml_cutensornet_amd as Q

    rng = np.random.default_rng(5)
    out = []
    for k in range(count):
        m = Q.random_mps(N, [1, 2, 4, 8, 8, 4, 2, 1], rng)
        ts = [np.array(t) for t in m.tensors]
        low = (rng.standard_normal((8, RANK)) + 1j * rng.standard_normal((8, RANK))) @ (rng.standard_normal((RANK, 8)) + 1j * rng.standard_normal((RANK, 8)))
        ts[RANK_BOND - 1] = np.tensordot(ts[RANK_BOND - 1], low, axes=(2, 0))
        out.append(scrambled(Q.MPS(ts), rng, scale=(3.7, 0.21, 1.0)[k % 3]))
    return out


def program_gates(unitary_only=False):
    u = haar(np.random.default_rng(9), 4)
    head = [("Ry", [q], [0.1 + 0.13 * q]) for q in range(N)] + [("Unitary2q", [2, 3], [u]), ("XXPhase", [4, 5], [0.3]), ("Rz", [3], [0.4])]
    assert len(head) == MEASURE
    mid = [] if unitary_only else [("Measure", [3], []), ("X", [5], [], (MEASURE, 1)), ("Depolarizing2q", [1, 2], [0.4])]
    return head + mid + [("ZZPhase", [5, 6], [0.4]), ("YYPhase", [0, 1], [0.25]), ("Rx", [6], [0.2])]


def dense_runs(n, gates, psi0):
    """Every classical record of an unrouted gate list applied to the vector psi0, and the unnormalised vector it leaves."""
    runs = [({}, np.asarray(psi0, dtype=complex).reshape((2,) * n))]
    for pos, g in enumerate(gates):
        name, qubits, params = g[:3]
        cond = g[3] if len(g) == 4 else None
        ms, is_channel = _matrices(name, params)
        nxt = []
        for rec, v in runs:
            if cond is not None and not (rec[cond[0]] >= 0 and rec[cond[0]] == cond[1]):
                nxt.append(({**rec, pos: -2} if is_channel else rec, v))
            elif is_channel:
                nxt.extend(({**rec, pos: b}, apply_dense(v, m, list(qubits))) for b, m in enumerate(ms))
            else:
                nxt.append((rec, apply_dense(v, ms[0], list(qubits))))
        runs = nxt
    return {tuple(rec[p] for p in sorted(rec)): v.reshape(-1) for rec, v in runs}


def run(c, builder, **kw):
    from qml_cutensornet_amd import mps

    if builder == "numpy":
        return mps._simulate(c, 1.0, 1e-16, None, None, **kw)
    return mps.simulate_native(c, 1.0, 1e-16, None, **kw)


def left_residual(t):
    m = t.reshape(-1, t.shape[2])
    return float(np.abs(m.conj().T @ m - np.eye(m.shape[1])).max())


def right_residual(t):
    m = t.reshape(t.shape[0], -1)
    return float(np.abs(m @ m.conj().T - np.eye(m.shape[0])).max())


def loop_centre(c, k):
    """Where the builders' loop has its orthogonality centre after k gates of an unconditional program from |0...0>: a channel on q
    brings it onto q, a two-qubit gate on (q, q + 1) leaves it on q + 1 unless the next two-qubit gate lies to the left of q."""
    from qml_cutensornet_amd.ansatz import is_two_qubit

    two = [int(q) for o, q in zip(c.op, c.q0) if is_two_qubit(int(o))]
    centre, g2 = 0, 0
    for o, q in zip(c.op[:k].tolist(), c.q0[:k].tolist()):
        if o == 10:
            centre = q
        elif is_two_qubit(o):
            g2 += 1
            centre = q + 1 if (two[g2] if g2 < len(two) else q) >= q else q
    return centre


# ---- seed_state
def test_seed_state_is_canonical_normalised_and_rank_revealing(built):
    from qml_cutensornet_amd import mps

    for m in input_states():
        assert m.bond_dims()[RANK_BOND] == 8
        v = mps_vector(m)
        # the gauge of ``scrambled`` (cond <= 4) leaves rounding of about 1e-15 of the norm in the directions a bond does not need
        # (tests/test_compress_host.py): the rank is defined for a zero above that noise, 1e-12 as there
        for zero in (1e-16, 1e-12):
            s, norm = mps.seed_state(m, zero)
            assert max(left_residual(t) for t in s.tensors[:-1]) <= 1e-12
            w = mps_vector(s)
            assert abs(np.vdot(w, w).real - 1) <= 1e-14
            assert (s.bond_dims() <= m.bond_dims()).all()
            assert abs(norm - math.sqrt(np.vdot(v, v).real)) <= 1e-12 * norm
            assert np.abs(w - v / norm).max() <= 1e-12  # the same vector, phase included
            assert abs(s.fidelity - 1) <= 1e-12 and s.logw == 0.0
        assert s.bond_dims()[RANK_BOND] == RANK


# ---- against the dense vector
@pytest.mark.parametrize("builder", BUILDERS)
def test_unitary_program_on_given_states_matches_the_dense_vector(built, builder):
    gates = program_gates(unitary_only=True)
    c = from_gates(N, gates)
    for m in input_states():
        v = mps_vector(m)
        (want,) = dense_runs(N, gates, v / np.linalg.norm(v)).values()
        got = run(c, builder, initial=m)
        assert np.abs(mps_vector(got) - want).max() <= 1e-12 and abs(got.fidelity - 1) <= 1e-12 and got.logw == 0.0


@pytest.mark.parametrize("builder", BUILDERS)
def test_branches_and_log_weights_on_given_states_match_the_dense_vector(built, builder):
    gates = program_gates()
    c = from_gates(N, gates)
    assert {8, 9, 10, 11} <= set(c.op.tolist()) and int(np.count_nonzero(c.cond_gate >= 0)) == 1
    seen = set()
    for s, m in enumerate(input_states()):
        v = mps_vector(m)
        want = dense_runs(N, gates, v / np.linalg.norm(v))
        assert abs(sum(np.vdot(p, p).real for p in want.values()) - 1) <= 1e-12
        for t in range(6):
            got, margin = run(c, builder, seed=SEED, state_index=s, trajectory=t, margin=True, initial=m)
            assert margin >= 1e-6  # no draw of the host sits at a threshold: the record is the dense simulator's too
            phi = want[tuple(int(b) for b in got.branches)]
            p = np.vdot(phi, phi).real
            assert abs(math.exp(got.logw) - p) <= 1e-12 and abs(got.logw - math.log(p)) <= 1e-12
            assert np.abs(mps_vector(got) - phi / math.sqrt(p)).max() <= 1e-12
            seen.add(tuple(int(b) for b in got.branches))
    assert {r[0] for r in seen} == {0, 1}  # the Measure came out both ways: the conditional X ran and was skipped


def test_numpy_and_native_agree_on_given_states(built):
    c = from_gates(N, program_gates())
    for s, m in enumerate(input_states()):
        for t in range(3):
            a = run(c, "numpy", seed=SEED, state_index=s, trajectory=t, initial=m)
            b = run(c, "native", seed=SEED, state_index=s, trajectory=t, initial=m)
            assert np.array_equal(a.branches, b.branches) and np.array_equal(a.bond_dims(), b.bond_dims())
            assert abs(a.fidelity - b.fidelity) <= 1e-12 and abs(a.logw - b.logw) <= 1e-12
            assert abs(np.vdot(mps_vector(a), mps_vector(b))) ** 2 >= 1 - 1e-12


# ---- the split identity, and the bit-for-bit resume
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("k", [3, 8, MEASURE])
def test_split_identity(built, builder, k):
    c = from_gates(N, program_gates())
    n_gates = c.n_gates
    for t in range(3):
        whole = run(c, builder, seed=SEED, trajectory=t)
        first = run(c.sliced(0, k), builder, seed=SEED, trajectory=t)
        second = run(c.sliced(k, n_gates), builder, seed=SEED, trajectory=t, first_gate=k, initial=first)
        assert np.array_equal(whole.branches, second.branches)  # every channel gate lies behind the cut
        assert abs(np.vdot(mps_vector(whole), mps_vector(second))) ** 2 >= 1 - 1e-10
        assert abs(whole.logw - second.logw) <= 1e-10


def test_initial_centre_resumes_the_numpy_loop_bit_for_bit(built):
    from qml_cutensornet_amd import mps

    c = from_gates(N, program_gates())
    n_gates = c.n_gates
    for k in (8, MEASURE):  # behind the Unitary2q (the centre on site 3), and behind the XXPhase
        cps = sorted({k, MEASURE + 2, n_gates - 1, n_gates})
        snaps = mps._simulate(c, 1.0, 1e-16, None, cps, seed=SEED, trajectory=1)
        j = cps.index(k)
        centre = loop_centre(c, k)
        s = snaps[j]
        assert max([left_residual(t) for t in s.tensors[:centre]] + [right_residual(t) for t in s.tensors[centre + 1:]] + [0.0]) <= 1e-12
        later = [x - k for x in cps[j + 1:]]
        again = mps._simulate(c.sliced(k, n_gates), 1.0, 1e-16, None, later, seed=SEED, trajectory=1, first_gate=k, initial=s, initial_centre=centre)
        assert len(again) == len(snaps) - j - 1
        for a, b in zip(again, snaps[j + 1:]):
            assert all(np.array_equal(x, y) for x, y in zip(a.tensors, b.tensors))
            assert a.fidelity == b.fidelity and a.logw == b.logw and np.array_equal(a.branches, b.branches)
        # through simulate(), and through the native builder: the same state
        one = mps.simulate(c.sliced(k, n_gates), 1.0, 1e-16, checkpoints=later, seed=SEED, trajectory=1, first_gate=k, initial=s, initial_centre=centre)[-1]
        assert all(np.array_equal(x, y) for x, y in zip(one.tensors, snaps[-1].tensors))
        nat = mps.simulate_native(c.sliced(k, n_gates), 1.0, 1e-16, seed=SEED, trajectory=1, first_gate=k, initial=s, initial_centre=centre)
        assert np.array_equal(nat.branches, snaps[-1].branches) and abs(nat.logw - snaps[-1].logw) <= 1e-12
        assert abs(np.vdot(mps_vector(nat), mps_vector(snaps[-1]))) ** 2 >= 1 - 1e-12


def test_initial_centre_carries_fidelity_and_log_weight(built):
    import qml_cutensornet_amd as Q
    from qml_cutensornet_amd import mps

    s, _ = mps.seed_state(input_states(1)[0])
    given = Q.MPS(s.tensors, 0.75, -1.5)
    c = from_gates(N, program_gates(unitary_only=True))
    for builder in BUILDERS:
        got = run(c, builder, initial=given, initial_centre=N - 1)
        assert abs(got.fidelity - 0.75) <= 1e-12 and got.logw == -1.5
        seeded = run(c, builder, initial=given)  # seeded: the sweep's fidelity, log-weight 0
        assert abs(seeded.fidelity - 1) <= 1e-12 and seeded.logw == 0.0


def test_initial_none_is_the_call_without_it(built):
    from qml_cutensornet_amd import mps

    c = from_gates(N, program_gates())
    for fn in (mps.simulate, mps.simulate_native, lambda *a, **kw: mps._simulate(*a, None, None, **kw)):
        a = fn(c, 1.0, 1e-16, seed=SEED, trajectory=2)
        b = fn(c, 1.0, 1e-16, seed=SEED, trajectory=2, initial=None, initial_centre=None)
        assert all(np.array_equal(x, y) for x, y in zip(a.tensors, b.tensors))
        assert a.fidelity == b.fidelity and a.logw == b.logw and np.array_equal(a.branches, b.branches)
    snaps = mps.simulate(c, 1.0, 1e-16, checkpoints=[4, c.n_gates], seed=SEED)
    again = mps.simulate(c, 1.0, 1e-16, checkpoints=[4, c.n_gates], seed=SEED, initial=None)
    assert all(np.array_equal(x, y) for a, b in zip(snaps, again) for x, y in zip(a.tensors, b.tensors))


# ---- rejections
@pytest.mark.parametrize("builder", BUILDERS + ["simulate"])
def test_rejections_by_name(built, builder):
    import qml_cutensornet_amd as Q
    from qml_cutensornet_amd import mps

    c = from_gates(N, program_gates(unitary_only=True))
    m = input_states(1)[0]
    go = (lambda **kw: mps.simulate(c, 1.0, 1e-16, **kw)) if builder == "simulate" else (lambda **kw: run(c, builder, **kw))
    with pytest.raises(ValueError, match="initial must be an MPS"):
        go(initial=m.tensors)
    with pytest.raises(ValueError, match="6 sites, the circuit 7 qubits"):
        go(initial=Q.random_mps(6, [1, 2, 2, 2, 2, 2, 1], np.random.default_rng(0)))
    for bad in (-1, N, 2.0, True):
        with pytest.raises(ValueError, match="initial_centre must be a site in 0 .. 6"):
            go(initial=m, initial_centre=bad)
    with pytest.raises(ValueError, match="initial_centre goes with an initial state"):
        go(initial_centre=2)
    nan = m.copy()
    nan.tensors[3][1, 0, 2] = complex(float("nan"), 0.0)
    with pytest.raises(ValueError, match="not finite"):
        go(initial=nan)
    with pytest.raises(ValueError, match="not finite"):
        go(initial=nan, initial_centre=3)
    with pytest.raises(ValueError, match="not finite"):
        go(initial=Q.MPS(m.tensors, float("inf")), initial_centre=3)
    zero = m.copy()
    zero.tensors[2] = np.zeros_like(zero.tensors[2])
    with pytest.raises(ValueError, match="norm 0"):
        go(initial=zero)


def _native_initial(lib, dims, tensors, centre, fidelity=1.0, logw=0.0):
    """``qkb_simulate_program`` on a one-gate program without tables, from the given state: (return code, error text, ...)."""
    from qml_cutensornet_amd import program as P

    op, q0, alpha = np.array([0], dtype=np.int8), np.array([0], dtype=np.int32), np.zeros(1)
    n = N
    dims = None if dims is None else np.ascontiguousarray(dims, dtype=np.int32)
    flat = np.ascontiguousarray(tensors, dtype=np.complex128)
    out_dims = np.zeros(n + 1, dtype=np.int32)
    prog = P.fill_program(1, n, op, q0, alpha)
    run = P.sized(P.QkbRun, trunc_budget=0.0, value_of_zero=1e-16, init_dims=None if dims is None else dims.ctypes.data, init_tensors=flat.ctypes.data, init_centre=centre,
                  init_fidelity=fidelity, init_logw=logw)
    res = P.sized(P.QkbResult, dims=out_dims.ctypes.data)
    rc = lib.qkb_simulate_program(C.byref(prog), C.byref(run), C.byref(res))
    if rc == 0:
        lib.qkb_free(res.tensors)
    return rc, lib.qkb_last_error().decode(), out_dims, res.fidelity, res.logw


def test_native_entry_rejections_and_the_null_table(built):
    from qml_cutensornet_amd import mps

    lib = mps._native_builder()
    assert lib is not None and hasattr(lib, "qkb_simulate_program")
    s, _ = mps.seed_state(input_states(1)[0])
    dims = s.bond_dims()
    flat = np.concatenate([t.ravel() for t in s.tensors])
    rc, _, out_dims, fid, lw = _native_initial(lib, dims, flat, N - 1, 0.5, -0.25)
    assert rc == 0 and np.array_equal(out_dims, dims) and fid == 0.5 and lw == -0.25
    rc, _, out_dims, fid, _ = _native_initial(lib, None, flat, 0)  # a null table: from |0...0>
    assert rc == 0 and out_dims.tolist() == [1] * (N + 1) and fid == 1.0
    for bad, text in ((0, "boundary bonds must be 1"), (N, "boundary bonds must be 1")):
        d = dims.copy()
        d[bad] = 2
        rc, err, *_ = _native_initial(lib, d, flat, 0)
        assert rc == -8 and text in err
    for v in (0, -3):
        d = dims.copy()
        d[2] = v
        rc, err, *_ = _native_initial(lib, d, flat, 0)
        assert rc == -8 and "bonds must be positive" in err
    for centre in (-1, N):
        rc, err, *_ = _native_initial(lib, dims, flat, centre)
        assert rc == -8 and "outside the register" in err
    for where in (0, flat.shape[0] - 1):
        f = flat.copy()
        f[where] = complex(0.0, float("inf"))
        rc, err, *_ = _native_initial(lib, dims, f, 0)
        assert rc == -8 and "not finite" in err
    rc, err, *_ = _native_initial(lib, dims, flat, 0, float("nan"))
    assert rc == -8 and "not finite" in err


# ---- the drivers' host side
def test_host_share_and_pools_pass_initial_states_on(built):
    import qml_cutensornet_amd as Q
    from qml_cutensornet_amd import mps
    from qml_cutensornet_amd.builder_pool import build_states
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import _initial_states, _simulate_share
    from test_feature_map_host import zz_template

    ans = Q.CircuitAnsatz(N, list(zz_template(N, 2, 0.8, 2)))
    X = np.random.default_rng(3).uniform(0.0, 1.0, (4, N))
    inputs = input_states(4)
    want = [mps_vector(mps.simulate(ans.circuit_for_data(x), 1 - 1e-16, initial=m)) for x, m in zip(X, inputs)]
    same = lambda states: all(abs(np.vdot(mps_vector(s), w)) ** 2 >= 1 - 1e-12 for s, w in zip(states, want))  # noqa: E731
    for rank, (lo, hi) in enumerate(((0, 2), (2, 4))):  # two ranks: each takes the initial states of its own points
        first, states, _, fid = _simulate_share(ans, X, rank, 2, 1 - 1e-16, False, "X", want_set=False, initial=_initial_states(inputs, 4, ans))
        assert first == lo and len(states) == hi - lo and all(abs(f - 1) < 1e-12 for f in fid)
        assert all(abs(np.vdot(mps_vector(s), w)) ** 2 >= 1 - 1e-12 for s, w in zip(states, want[lo:hi]))
    assert same(build_states(ans, X, 1 - 1e-16, workers=2, initial=inputs)[0]) and same(build_states(ans, X, 1 - 1e-16, workers=1, initial=inputs)[0])
    assert same(mps.simulate_many([ans.circuit_for_data(x) for x in X], 1 - 1e-16, workers=2, initial=inputs)[0])
    one = mps.simulate_many([ans.circuit_for_data(x) for x in X], 1 - 1e-16, workers=2, initial=inputs[0])[0]  # one state for all
    assert abs(np.vdot(mps_vector(one[3]), mps_vector(mps.simulate(ans.circuit_for_data(X[3]), 1 - 1e-16, initial=inputs[0])))) ** 2 >= 1 - 1e-12
    # None is the call without it, for any ansatz (one that does not say how many qubits it has included)
    assert _initial_states(None, 4, object()) is None and _initial_states(inputs[0], 4, object()) is inputs[0]
    plain = _simulate_share(ans, X, 0, 1, 1 - 1e-16, False, "X", want_set=False)[1]
    again = _simulate_share(ans, X, 0, 1, 1 - 1e-16, False, "X", want_set=False, initial=None)[1]
    assert all(np.array_equal(a, b) for s, t in zip(plain, again) for a, b in zip(s.tensors, t.tensors))
    for bad, text in ((inputs[:3], "one per data point"), ([m.tensors for m in inputs], "one per data point"), (Q.random_mps(5, [1, 2, 2, 2, 2, 1], np.random.default_rng(0)), "7 sites")):
        with pytest.raises(ValueError, match=text):
            _initial_states(bad, 4, ans)
    with pytest.raises(ValueError, match="3 initial states for 4"):
        mps.simulate_many([ans.circuit_for_data(x) for x in X], 1 - 1e-16, initial=inputs[:3])
    with pytest.raises(ValueError, match="3 initial states for 4"):
        build_states(ans, X, 1 - 1e-16, initial=inputs[:3])
