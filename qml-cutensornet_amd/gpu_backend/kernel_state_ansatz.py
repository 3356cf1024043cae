"""MI355X drop-in for the reference module of the same name.

Surface kept (reference: /root/reference/gpu_backend/kernel_state_ansatz.py):
  * ``KernelStateAnsatz(num_qubits, reps, gamma, entanglement_map, hadamard_init=True)``  (ref :16-103)
  * ``build_kernel_matrix(mpi_comm, ansatz, X, Y=None, info_file=None, truncation_error=None,
    loglevel=30) -> np.ndarray``                                                          (ref :106-452)
    same argument meaning, same exceptions (ref :136-139), same orientation
    ``K[len(Y) or len(X), len(X)]`` with rows = Y (ref :325-326, :387), valid on rank 0,
    same profiling-JSON keys (ref :160-162, 205, 238-244, 301-320, 434-444).

What differs is how the work is done: the reference loops over pairs in Python and calls
cuTensorNet once per entry, rotating pickled MPS between ranks; here a rank builds its share of
the states, keeps it as ONE packed device image, the images are exchanged as flat buffers (one
RCCL all-gather, ``dist.exchange_sets``) so that every rank holds all MPS on its MI355X, each
rank sweeps its share of the pairs in one persistent HIP kernel launch and the shares meet in a
single all-gather (RCCL through torch.distributed when it is initialised with the nccl backend,
the communicator's own ``allgather`` otherwise).

The ``build_*`` drivers share their plumbing, each concern in one place: ``_checked_points`` raises the two argument errors every
driver has and casts the data; ``_start`` is the run prologue (rank, device, host cores, context, clock: a ``_Run``), called after
a driver's own argument checks; ``_chunk`` is the share arithmetic of the three share builders; ``_build_shares`` builds X then Y
as device sets and ``_share_features`` turns one share into a feature array and closes it; ``_exchanged`` lends the full sets and
closes what the exchange made; ``_profile_head``, ``_sim_stats``, ``_chi_stats`` and ``_write_profile`` make the profiling JSON.
"""
from __future__ import annotations

import json
import sys
import time
from contextlib import contextmanager
from statistics import mean, median
from typing import NamedTuple

import numpy as np

try:  # normal case: imported as qml_cutensornet_amd.gpu_backend.kernel_state_ansatz
    from ..ansatz import OP_K2, OP_M2, OP_XX, OP_YY, OP_ZZ, KernelStateAnsatz, as_bound_circuit, check_depths, reject_channels  # noqa: F401
    from .. import engine as _engine
    from ..dist import assemble_gram, comm_allgather, exchange_sets
    from ..mps import MPS, simulate, simulate_many  # noqa: F401
except ImportError:  # imported top-level as gpu_backend.kernel_state_ansatz
    import qml_cutensornet_amd as _pkg  # noqa: F401
    from qml_cutensornet_amd.ansatz import OP_K2, OP_M2, OP_XX, OP_YY, OP_ZZ, KernelStateAnsatz, as_bound_circuit, check_depths, reject_channels  # noqa: F401
    from qml_cutensornet_amd import engine as _engine
    from qml_cutensornet_amd.dist import assemble_gram, comm_allgather, exchange_sets
    from qml_cutensornet_amd.mps import MPS, simulate, simulate_many  # noqa: F401

ROOT_RANK = 0


def _say(is_root, text):
    if is_root:
        print(text)
        sys.stdout.flush()


class _Run(NamedTuple):
    """What a driver knows once it has started: who this rank is, its device and context, its share of the host cores, the clock."""
    rank: int
    n_procs: int
    is_root: bool
    device_id: int
    host_workers: int
    ctx: object
    t_start: float


def _start(mpi_comm, what):
    """The prologue of every driver, after its argument checks: ranks share the devices round robin (device = rank % n_devices,
    ref :152) and the host cores of the node.  ``what`` is the subject of the error without a device ("the Gram path has")."""
    rank, n_procs = mpi_comm.Get_rank(), mpi_comm.Get_size()
    n_dev = _engine.device_count()
    if n_dev <= 0:
        raise _engine.QkError(f"no gfx950 device visible: {what} no CPU fallback")
    from qml_cutensornet_amd import builder_pool

    host_workers = max(1, builder_pool.default_workers() // max(1, min(n_procs, n_dev)))  # host cores of this rank's share of the node
    return _Run(rank, n_procs, rank == ROOT_RANK, rank % n_dev, host_workers, _engine.default_context(rank % n_dev), time.perf_counter())


def _chunk(n, rank, n_procs):
    """(lo, hi) of this rank's slice of n points: contiguous chunks of ceil(n / n_procs), as ref :154,:171-174."""
    per_rank = -(-n // n_procs)
    lo = min(n, rank * per_rank)
    return lo, min(n, lo + per_rank)


def _checked_points(X, Y, truncation_error):
    """The two argument errors of the reference (ref :136-139) -> (X, Y or None, fidelity), the data as float64."""
    if Y is not None and len(X) < len(Y):
        raise ValueError("X must not be smaller than Y. Swap input order and transpose output.")
    if truncation_error is None:
        raise ValueError("You must specify a truncation error.")
    return np.asarray(X, dtype=np.float64), None if Y is None else np.asarray(Y, dtype=np.float64), 1.0 - float(truncation_error)


def _close_all(sets):
    for s in sets:
        if s is not None:
            s.close()


_PILOT_MIN_STATES = 24  # below this a share goes to the device builder as a whole (states that outgrow the cap: host)


def _entangling_weight(circuit):
    """Cost proxy of a circuit: sum of sin^2(pi alpha) over its XXPhase, YYPhase and ZZPhase gates (alpha in half-turns:
    0 and 1 do not entangle), plus 1 -- the most such a gate can add -- for every 4x4 matrix gate and every two-qubit Kraus channel (op
    codes 9 and 11: their entangling
    power is not worth a decomposition here, and without the term a circuit of matrix gates would weigh 0 and always be
    expected to keep small bonds).  It tracks the bonds a state will reach.  The device builder orders its queue by the
    first part alone: the matrix gates of the states of one call share their positions, so the constant would not reorder them.
    With a shared table all states of a share weigh the same, which the policies below read as "equally expensive":
    ``_auto_builder`` decides by the size of the share, and ``_hybrid_build`` sends every state the pilot's lightest dropped one
    does not outweigh to the host -- all of them, if the pilot drops any."""
    op = np.asarray(circuit.op)
    xx = np.isin(op, (OP_XX, OP_YY, OP_ZZ))
    return float((np.sin(np.pi * np.asarray(circuit.alpha)[xx]) ** 2).sum()) + float(np.count_nonzero((op == OP_M2) | (op == OP_K2)))


def _hybrid_build(ctx, circuits, fidelity, cap, host_workers, is_root, label):
    """QK_BUILDER=hybrid for a large share: the device builder (bonds capped at ``cap``) and the host pool work AT THE SAME
    TIME, and a state predicted to outgrow the cap never visits the device.
      1. the heaviest quarter (by the cost proxy) starts on the host pool at once -- whatever the prediction will say,
         these are the states the host is the better tool for;
      2. meanwhile a pilot of 8 states spread over the rest runs on the device (partial): the lightest state it drops
         sets the threshold of the prediction;
      3. predicted-to-fit states go to the device in one launch while the host pool takes the others;
      4. what the device still drops (misprediction) is built on the host at the end.
    Returns (list[MPS], seconds per state), or None when the device builder fails (the caller falls back)."""
    import threading

    m = len(circuits)
    w = np.array([_entangling_weight(c) for c in circuits])
    order = np.argsort(w)  # lightest first
    states, secs = [None] * m, [0.0] * m

    def host(idx, box):
        t0 = time.perf_counter()
        built, bsecs = simulate_many([circuits[k] for k in idx], fidelity, workers=host_workers)
        for k, mps, dt in zip(idx, built, bsecs):
            states[k], secs[k] = mps, dt
        box.append(time.perf_counter() - t0)

    def device(idx):
        t0 = time.perf_counter()
        built, info = ctx.build_mps([circuits[k] for k in idx], fidelity, max_bond=cap, partial=True)
        dt = (time.perf_counter() - t0) / max(1, len(idx))
        dropped = []
        for pos, k in enumerate(idx):
            if built[pos] is None:
                dropped.append(k)
            else:
                states[k], secs[k] = built[pos], dt
        return dropped

    heavy = [int(k) for k in order[m - m // 4 :]]
    rest = [int(k) for k in order[: m - m // 4]]
    pilot = sorted({rest[int(round(f * (len(rest) - 1)))] for f in np.linspace(0.0, 1.0, 8)})
    box_a = []
    th = threading.Thread(target=host, args=(heavy, box_a))
    th.start()
    try:
        pilot_dropped = device(pilot)
    except _engine.QkError as exc:
        th.join()
        _say(is_root, f"{label}: device builder gave up on the pilot ({exc}); building on the host")
        return None
    thr = min((w[k] for k in pilot_dropped), default=np.inf)  # lightest state the device could not hold
    others = [k for k in rest if k not in pilot]
    dev_idx = [k for k in others if w[k] < thr]
    host_idx = [k for k in others if w[k] >= thr] + pilot_dropped
    _say(is_root, f"{label}: pilot of {len(pilot)}: {len(pilot_dropped)} outgrew bond {cap}; device builder takes {len(dev_idx)} states, host pool {len(heavy) + len(host_idx)}")
    th.join()
    box_b = []
    th = threading.Thread(target=host, args=(host_idx, box_b)) if host_idx else None
    if th:
        th.start()
    late = []
    try:
        if dev_idx:
            late = device(dev_idx)
    except _engine.QkError as exc:
        _say(is_root, f"{label}: device builder gave up ({exc}); its states go to the host")
        late = dev_idx
    if th:
        th.join()
    if late:
        host(late, [])
    return states, secs


def _auto_builder(circuits, host_workers):
    """QK_BUILDER=auto: device or host for this share, from its size, the host cores at hand and the spread of the cost proxy.
    Calibration (one MI355X box with a 16-core share, profiles/r03/builder_policy.txt): the device builder runs a state per
    workgroup -- 256 to 1024 in flight -- and a launch ends with its heaviest state, which takes about 2.5 x what one host
    core needs for it (60 qubits x 6 layers, gamma = 1: 4.3 s for the longest of 500 states, whose sum is 230-430 cpu-s).
    The host pool needs (states x mean cost) / workers.  With the heaviest state at (w_max / w_mean)^2 times the mean cost the
    device wins from about 2.5 x workers x (w_max / w_mean)^2 states on -- at 16 workers: 137 states of that config (ratio 1.85),
    250 of the 100-qubit gamma = 0.1 one (2.5), 180 of the 40-qubit x 4-layer one (2.1): the full data sets go to the device, an
    eighth of the 60-qubit one (63 states) stays on the host cores."""
    m = len(circuits)
    if m == 0:
        return "host"
    w = np.array([_entangling_weight(c) for c in circuits])
    ratio = float(w.max() / w.mean()) if w.mean() > 0 else 1.0
    need = 2.5 * max(1, host_workers) * max(1.0, ratio) ** 2
    return "device" if m >= need else "host"


SMALL_BOND_CAP = 64  # the device builder's cap for shares whose bonds are expected to stay small (_expect_small_bonds)


def _expect_small_bonds(ansatz, circuits):
    """Will the bonds of this share stay small (a few tens)?  Then the device builder's 256-thread shape with two workgroups per CU
    (512 states in flight, most factorisations in LDS; bond cap 64) is the right one -- 100 qubits x 10 layers at gamma = 0.1
    (final bonds <= 32, a few more in mid-circuit): 1000 states -- against one 512-thread workgroup per CU, the shape for bonds in
    the hundreds (17.9 s for the same 1000 states).  Yes when the analytic bound 2^(distance x layers) says so, or when the
    heaviest circuit's entangling weight is small (calibration: 40 qubits x 4 layers at gamma = 0.5, bonds 20-26, has w_max = 8.4;
    gamma = 1 configurations start at w = 11 and reach bonds 60-250).  A wrong yes costs one short launch: a state that outgrows
    the small cap is dropped at the gate where it does and the share is rebuilt with the large one."""
    try:
        dist_max = max((abs(int(b_) - int(a_)) for a_, b_ in ansatz.entanglement_map), default=0)
        if 2 ** min(dist_max * int(ansatz.reps), int(ansatz.num_qubits) // 2) <= 64:
            return True
    except (AttributeError, TypeError, ValueError):
        pass
    return max(_entangling_weight(c) for c in circuits) <= 10.0


def _initial_states(initial_states, n_points, ansatz, name="initial_states"):
    """``initial_states`` of a driver, checked: ``None``, one ``MPS`` for every data point, or a list of ``MPS``, one per point, each
    with as many sites as the ansatz has qubits (an ansatz that does not say is checked by the builder)."""
    from qml_cutensornet_amd.mps import MPS

    if initial_states is None:
        return None
    n_qubits = getattr(ansatz, "num_qubits", None)
    if isinstance(initial_states, MPS):
        states = [initial_states]
    else:
        states = list(initial_states)
        if len(states) != n_points or not all(isinstance(m, MPS) for m in states):
            raise ValueError(f"{name} must be one MPS, or a list of MPS with one per data point ({n_points})")
        initial_states = states
    if n_qubits is not None and any(len(m) != int(n_qubits) for m in states):
        raise ValueError(f"{name}: every initial state needs {n_qubits} sites, as many as the ansatz has qubits")
    return initial_states


def _share_of(initial, lo, hi):
    """The initial states of the points lo .. hi-1: the one state for all, or the slice of the list."""
    return initial if initial is None or not isinstance(initial, list) else initial[lo:hi]


def _simulate_share(ansatz, points, rank, n_procs, fidelity, is_root, label, device_id=0, host_workers=1, want_set=True, initial=None):
    """This rank's slice of the data set (contiguous chunks of ceil(N/P), as ref :154,:171-174) -> (first index, the
    states as ONE packed device set -- ``None`` for an empty share --, seconds per state, fidelities).  ``want_set=False``
    (host-only callers: the CPU tests) keeps the host builder's list of MPS instead of uploading it.
    QK_MAX_BOND (environment): a bond cap for either builder -- the ``chi`` pytket-cutensornet's ``Config`` would take at
    ref :141-144 (the reference leaves it unset: the default is no cap).

    ``initial`` (``_initial_states``: one MPS, or one per point of ``points``) starts the circuits from given states instead of
    |0...0>.  Then "auto" and "hybrid" build the whole share on the device, and a share the device gives up on is rebuilt on the
    host as a whole (the rule of the noisy drivers: no per-state hand-over); "host" is ``simulate(..., initial=)``."""
    import os

    lo, hi = _chunk(len(points), rank, n_procs)
    chi = int(os.environ.get("QK_MAX_BOND", "0")) or None
    which = os.environ.get("QK_BUILDER", "auto") if want_set else "host"  # auto | device | hybrid | host
    forced = which  # what the caller asked for: only a FORCED device build may fail the call
    # an ansatz may return a BoundCircuit or a reference-style gate list (name, qubits, params)
    circuits = [as_bound_circuit(ansatz.circuit_for_data(points[k, :]), ansatz) for k in range(lo, hi)] if hi > lo else []
    reject_channels(circuits, "a driver without trajectories")
    inits = _share_of(initial, lo, hi)
    if inits is not None and hi > lo:
        if which != "host":
            t0 = time.perf_counter()
            cap = chi or int(os.environ.get("QK_BUILDER_MAX_BOND", "320"))
            try:
                dset, _, binfo = _engine.default_context(device_id).build_share(circuits, fidelity, max_bond=cap, truncate=chi is not None, initial=inits)
                _say(is_root, f"{label}: 100%")
                return lo, dset, [(time.perf_counter() - t0) / (hi - lo)] * (hi - lo), [float(f) for f in binfo["fidelity"]]
            except _engine.QkError as exc:
                if forced == "device":
                    raise
                _say(is_root, f"{label}: device builder gave up ({exc}); building on the host")
        which = "host"
    elif which == "auto":
        try:
            which = _auto_builder(circuits, host_workers)
        except (AttributeError, TypeError, ValueError):  # an ansatz without a compiled gate program: the host loop handles it
            which = "host"
    if which in ("device", "hybrid") and hi > lo:
        # the rank's whole share in ONE launch of the device builder (csrc/qk_build.hip): what the reference does with
        # simulate(libhandle, ...) on the rank's GPU (ref :221,:263).  "device" / "auto": bonds up to QK_BUILDER_MAX_BOND (320:
        # bonds in mid-circuit exceed the final ones), a state that outgrows it is built on the host afterwards (a forced
        # "device" fails instead); "hybrid" caps at 64 and builds what outgrows the cap on the host pool -- concurrently, behind a
        # pilot, for shares of >= 24 states (_hybrid_build); "host" skips it.
        t0 = time.perf_counter()
        cap = chi or int(os.environ.get("QK_BUILDER_MAX_BOND", "64" if which == "hybrid" else "320"))
        partial = which == "hybrid" or (forced == "auto" and chi is None)
        ctx = _engine.default_context(device_id)
        if which == "hybrid" and hi - lo >= _PILOT_MIN_STATES and chi is None:
            out = _hybrid_build(ctx, circuits, fidelity, cap, host_workers, is_root, label)
            if out is not None:
                states, secs = out
                _say(is_root, f"{label}: 100%")
                return lo, ctx.upload(states), secs, [m.fidelity for m in states]
        try:
            dset = binfo = states = None
            if chi is None and cap > SMALL_BOND_CAP and which != "hybrid" and _expect_small_bonds(ansatz, circuits):
                dset, states, binfo = ctx.build_share(circuits, fidelity, max_bond=SMALL_BOND_CAP, partial=True)
                if dset is None:  # some state outgrew the small cap after all: the whole share again, with the large one
                    _say(is_root, f"{label}: {len(binfo['dropped'])} of {hi - lo} states outgrew bond {SMALL_BOND_CAP}; rebuilding with bonds up to {cap}")
                    dset = binfo = states = None
            if binfo is None:
                dset, states, binfo = ctx.build_share(circuits, fidelity, max_bond=cap, partial=partial, truncate=chi is not None)
        except _engine.QkError as exc:
            if forced == "device":
                raise
            _say(is_root, f"{label}: device builder gave up ({exc}); building on the host")
            dset, states, binfo = None, None, None
        if binfo is not None:
            dt = (time.perf_counter() - t0) / (hi - lo)
            secs = [dt] * (hi - lo)
            if dset is not None:  # every state fitted: the share is already a packed device set, nothing was downloaded
                _say(is_root, f"{label}: 100%")
                return lo, dset, secs, [float(f) for f in binfo["fidelity"]]
            if binfo["dropped"]:  # states whose bonds outgrew the cap: the host builder is the better tool for those
                _say(is_root, f"{label}: {len(binfo['dropped'])} of {hi - lo} states outgrew bond {cap}; building them on the host")
                built, bsecs = simulate_many([circuits[k] for k in binfo["dropped"]], fidelity, workers=host_workers)
                for k, m, dt_k in zip(binfo["dropped"], built, bsecs):
                    states[k], secs[k] = m, dt_k
            _say(is_root, f"{label}: 100%")
            return lo, ctx.upload(states), secs, [m.fidelity for m in states]
    # host builder: one circuit per core on a thread pool (no fork: the GPU may already be initialised; the native builder
    # releases the GIL) -- the reference's loop is serial because its simulate() runs on the GPU (ref :213-231)
    tick, done = max(1, (hi - lo) // 10), [0]  # (the root's share is a full chunk, and only the root prints)

    def progress():
        done[0] += 1
        if (done[0] - 1) % tick == 0:
            _say(is_root, f"{label}: {10 * ((done[0] - 1) // tick)}%")

    states, secs = simulate_many(circuits, fidelity, workers=host_workers, progress=progress, max_bond=chi, initial=inits)
    if not want_set:
        return lo, states, secs, [m.fidelity for m in states]
    if not states:
        return lo, None, secs, []
    return lo, _engine.default_context(device_id).upload(states), secs, [m.fidelity for m in states]


def _gram_on_device(comm, rank, n_procs, ctx, xset, yset):
    """The hot path.  Returns (K on the host or None, seconds in the final exchange)."""
    use_torch = False
    if n_procs > 1:
        try:
            import torch.distributed as dist

            use_torch = dist.is_initialized() and dist.get_world_size() == n_procs and dist.get_backend() == "nccl"
        except ImportError:
            use_torch = False
    if n_procs == 1:
        return ctx.gram(xset, yset), 0.0
    if use_torch:
        import importlib

        GramJob = importlib.import_module("qml_cutensornet_amd.gram").GramJob

        job = GramJob(ctx, xset, yset, n_procs, rank)
        t0 = time.perf_counter()
        K = job.run()
        job.close()
        return K, time.perf_counter() - t0
    # host communicator (mpi4py or gloo): sweep on the GPU, all-gather the packed values on the host
    plan = _engine.Plan(xset.dims, None if yset is None else yset.dims, n_procs, rank)
    vals = ctx.gram_values_host(xset, yset, plan)
    t0 = time.perf_counter()
    shares = comm_allgather(comm, (plan.pairs(), vals))
    exchange = time.perf_counter() - t0
    ny = len(xset) if yset is None else len(yset)
    K = assemble_gram(ny, len(xset), [s[0] for s in shares], [s[1] for s in shares], yset is None)
    plan.close()
    return K, exchange


def _set_mib(dims):
    """MiB of the complex128 tensors of the states with bond table ``dims`` (what the reference sums from .nbytes, ref :295)."""
    d = np.asarray(dims, dtype=np.float64)
    return float((32.0 * d[:, :-1] * d[:, 1:]).sum() / 2**20)


def _initial_pair(initial_states, initial_states_Y, X, Y, ansatz):
    """(``initial_states`` for X, ``initial_states_Y`` for Y), checked; the second is ``None`` without Y."""
    return (_initial_states(initial_states, len(X), ansatz),
            _initial_states(initial_states_Y if Y is not None else None, 0 if Y is None else len(Y), ansatz, "initial_states_Y"))


class _Share(NamedTuple):
    """This rank's share of a data set: the ``_simulate_share`` result behind its label and the size of the whole set.  ``_exchanged``
    reads ``lo`` and ``total`` only, so the two drivers with shares of another kind count them in their own unit: the noisy kernel in
    states (T per point), and the depth scan keeps {depth: set} and {depth: fidelities} where one set and one list stand here."""
    label: str
    total: int
    lo: int
    local: object  # the packed device set, None for an empty share
    secs: list
    fids: list


def _build_shares(run, ansatz, X, Y, fidelity, inits=None):
    """This rank's shares of X and Y (each unless None) as device sets, built in that order: [_Share, ...].  The caller closes the sets."""
    shares = []
    try:
        for k, (label, points) in enumerate((("X", X), ("Y", Y))):
            if points is not None:
                _say(run.is_root, f"\nContracting the MPS of the circuits from the {label} dataset...")
                built = _simulate_share(ansatz, points, run.rank, run.n_procs, fidelity, run.is_root, label, run.device_id, run.host_workers,
                                        initial=None if inits is None else inits[k])
                shares.append(_Share(label, len(points), *built))
    except BaseException:
        _close_all(s.local for s in shares)
        raise
    # the device builder keeps its per-workgroup arena and workspace on the context (tens of GB at large bond caps): they go back before
    # the exchange and the sweep need the memory (several ranks may share one GPU)
    run.ctx.trim()
    return shares


def _share_features(run, ansatz, points, label, fidelity, empty_shape, features_of, initial=None):
    """One data set of a driver that exchanges features, never states: this rank's share is built, ``features_of(set, first
    index)`` makes its float64 feature array (an empty share gets zeros of shape (0,) + empty_shape) and the set is closed.
    Returns (features, first index, largest bond of every state, seconds per state, fidelities, seconds in ``features_of``)."""
    _say(run.is_root, f"\nContracting the MPS of the circuits from the {label} dataset...")
    lo, local, secs, fids = _simulate_share(ansatz, points, run.rank, run.n_procs, fidelity, run.is_root, label, run.device_id, run.host_workers, initial=initial)
    run.ctx.trim()  # the device builder's arena goes back before the feature kernels need memory
    t0 = time.perf_counter()
    if local is None:
        F, chi = np.zeros((0,) + tuple(empty_shape), dtype=np.float64), np.zeros(0)
    else:
        try:
            F, chi = features_of(local, lo), local.dims.max(axis=1)
        finally:
            local.close()
    return F, lo, chi, secs, fids, time.perf_counter() - t0


def _gathered_features(run, mpi_comm, ansatz, X, Y, fidelity, empty_shape, features_of, inits=(None, None)):
    """``_share_features`` of X and (unless None) Y with ``features_of(label, set, first index)``, then the all-gathers: ([features of
    all of X, of all of Y], [largest bonds likewise], seconds per state, fidelities, seconds in the features, seconds in the gathers)."""
    parts, sim_secs, fids, feat_secs = [], [], [], 0.0
    for k, (label, points) in enumerate((("X", X), ("Y", Y))):
        if points is None:
            continue
        F, lo, chi, secs, fid, dt = _share_features(run, ansatz, points, label, fidelity, empty_shape,
                                                    lambda local, lo, label=label: features_of(label, local, lo), inits[k])
        parts.append((lo, F, chi, len(points)))
        sim_secs, fids, feat_secs = sim_secs + secs, fids + fid, feat_secs + dt
    t0 = time.perf_counter()
    feats = [_gather_features(mpi_comm, lo, F, total) for lo, F, _, total in parts]
    chi_all = [np.concatenate([np.asarray(c, dtype=np.float64) for c in comm_allgather(mpi_comm, chi)]) for _, _, chi, _ in parts]
    return feats, chi_all, sim_secs, fids, feat_secs, time.perf_counter() - t0


@contextmanager
def _exchanged(run, mpi_comm, locals_, shares):
    """The full sets of the local ones (``exchange_sets`` with each share's first index and total): every rank holds all states
    inside the block.  On exit the sets the exchange made are closed; a local set that came back as the full one (a single
    rank) is its owner's to close."""
    full = []
    try:
        for loc, s in zip(locals_, shares):
            full.append(exchange_sets(mpi_comm, run.ctx, loc, s.lo, s.total)[0])
        yield full
    finally:
        _close_all(f for f, loc in zip(full, locals_) if f is not loc)


def _gram_of(run, mpi_comm, full):
    """``_gram_on_device`` of the exchanged sets [X] or [X, Y]."""
    return _gram_on_device(mpi_comm, run.rank, run.n_procs, run.ctx, full[0], full[1] if len(full) > 1 else None)


def _profile_head(run, X, Y):
    return {"n_procs": [run.n_procs, "gpus"], "lenX": [len(X), "entries"], "lenY": [None if Y is None else len(Y), "entries"]}


def _sim_stats(sim_secs, quartiles=True):
    """The simulation entries of a profile.  (``quartiles=False``: ``build_shot_feature_kernel_matrix`` has never written q1 and
    q3, unlike its siblings; its JSON keeps the keys it has.)"""
    prof = {"r0_circ_sim": [sum(sim_secs), "seconds"]}
    if sim_secs:
        prof["avg_circ_sim"] = [mean(sim_secs), "seconds"]
        prof["median_circ_sim"] = [median(sim_secs), "seconds"]
        if quartiles:
            prof["q1_circ_sim"] = [float(np.percentile(sim_secs, 25)), "seconds"]
            prof["q3_circ_sim"] = [float(np.percentile(sim_secs, 75)), "seconds"]
    return prof


def _chi_stats(chi_all):
    """The mean largest bond of the states of X and of Y (``chi_all``: one array per data set; without Y, Y is X)."""
    return {f"ave max chi {v}": (float(chi.mean()) if chi.size else 0.0, f"chi {v}") for v, chi in (("x", chi_all[0]), ("y", chi_all[-1]))}


def _write_profile(info_file, prof):
    if info_file is not None:
        with open(info_file + ".json", "w") as fp:
            json.dump(prof, fp, indent=4)


def build_kernel_matrix(mpi_comm, ansatz, X, Y=None, info_file=None, truncation_error=None, loglevel=30, initial_states=None, initial_states_Y=None):
    """Fill the kernel (Gram) matrix ``K[j, i] = |<psi(X_i)|psi(Y_j)>|^2``; ``Y=None`` means ``Y = X``.

    Returns the ``len(Y) x len(X)`` float64 matrix on rank 0 and ``None`` elsewhere (the reference
    returns the result of ``reduce(..., root=0)``, ref :428,:452).

    ``initial_states`` (one ``MPS`` for all, or a list with one per data point of X; ``initial_states_Y`` for Y) applies the circuits
    to given states instead of |0...0> -- any gauge, any norm (``Context.seed``, ``mps.seed_state``).  ``None`` is the call without it.
    """
    X, Y, fidelity = _checked_points(X, Y, truncation_error)
    inits = _initial_pair(initial_states, initial_states_Y, X, Y, ansatz)
    run = _start(mpi_comm, "the Gram path has")
    prof = _profile_head(run, X, Y)
    prof["r0_circ_gen"] = [0.0, "seconds"]  # circuits are bound lazily inside the simulation loop; the reference times their generation apart
    shares = _build_shares(run, ansatz, X, Y, fidelity, inits)
    locals_ = [s.local for s in shares]
    try:
        t0 = time.perf_counter()
        # every rank gets the whole set: the packed device images of the shares, one all-gather (ref :341-352, 415-419)
        with _exchanged(run, mpi_comm, locals_, shares) as full:
            gather_secs = time.perf_counter() - t0
            if run.n_procs > 1:  # the full sets are copies: the shares go back before the sweep needs the memory
                _close_all(locals_)
            if run.is_root:
                sim_secs, fids = [t for s in shares for t in s.secs], [f for s in shares for f in s.fids]
                prof.update(_sim_stats(sim_secs))
                total_mib = sum(_set_mib(f.dims) for f in full)
                prof["gpu_mps_mem"] = [total_mib, "MiB"]  # every GPU holds the whole set here
                prof["avg_mps_mem"] = [total_mib / sum(len(f) for f in full), "MiB"]
                prof["avg_fidelity"] = [sum(fids) / max(1, len(fids)), ""]
                prof.update(_chi_stats([f.dims.max(axis=1) for f in full]))
                prof["r_nonRR_recv"] = [0, "seconds"]  # no ranks outside a ring: there is no ring
                prof["r0_RR_recv"] = [gather_secs, "seconds"]  # exchange of the packed sets; the Gram all-gather is added below
                _say(True, "\nFinished contracting all MPS.\n\nCalculating kernel matrix...")
            t_tiles = time.perf_counter()
            kernel_mat, exchange = _gram_of(run, mpi_comm, full)
            tiles = time.perf_counter() - t_tiles
    finally:
        _close_all(locals_)  # (a no-op for sets closed above: ``MpsSet.close`` may be called twice)

    if not run.is_root:
        return None
    n_entries = kernel_mat.size if Y is not None else len(X) * (len(X) + 1) // 2
    per_entry = tiles / max(1, n_entries)
    prof["r0_RR_recv"][0] += exchange
    prof["kernel_mat_time"] = [tiles, "seconds"]
    prof["total_time"] = [time.perf_counter() - run.t_start, "seconds"]
    # one launch computes every overlap: per-product statistics collapse to the mean
    prof["r0_product"] = [tiles - exchange, "seconds"]
    for key in ("avg_product", "median_product", "q1_product", "q3_product"):
        prof[key] = [per_entry, "seconds"]
    _say(True, f"\nFinished calculating all inner products.\n\tAverage time per inner product: {per_entry:.3e} seconds.\n")
    _write_profile(info_file, prof)
    return kernel_mat


def _gather_features(comm, lo, F, total):
    """All-gather of every rank's (first index, features of its share: Bloch vectors (m, n, 3) or pair correlators
    (m, n_pairs, 4, 4)) -> the (total, ...) array in data-set order."""
    shares = comm_allgather(comm, (int(lo), np.ascontiguousarray(F, dtype=np.float64)))
    out = np.zeros((total,) + tuple(F.shape[1:]), dtype=np.float64)
    for s_lo, s_F in shares:
        out[s_lo : s_lo + s_F.shape[0]] = s_F
    return out


def build_projected_kernel_matrix(mpi_comm, ansatz, X, Y=None, pqk_gamma=None, info_file=None, truncation_error=None, loglevel=30, rdm=1, pair_distance=1, observables=None,
                                  shots=None, shot_seed=0, window=False, initial_states=None, initial_states_Y=None):
    """Projected quantum kernel (Huang et al., Nat. Commun. 12, 2631 (2021)) of the same states as ``build_kernel_matrix``:
        K[j, i] = exp(-g sum_k ||rho_k(X_i) - rho_k(Y_j)||_F^2) = exp(-g/2 sum_k |F(X_i)[k] - F(Y_j)[k]|^2),
    rho_k = the one-qubit reduced density matrix of qubit k, F[k] = its Bloch vector (<X_k>, <Y_k>, <Z_k>); ``Y=None`` means
    ``Y = X``, ``pqk_gamma=None`` means g = 1 / n_qubits.  Each rank builds its share of the states (the builder policy of
    ``build_kernel_matrix``), computes their Bloch vectors on its device and all-gathers them (3 n reals per state, never an
    MPS); rank 0 computes K on its GPU and returns the ``len(Y) x len(X)`` matrix, the other ranks return ``None``.

    ``rdm=2`` is the two-qubit form on neighbouring qubits, the first projected kernel that sees correlations between qubits:
        K_2[j, i] = exp(-g sum_k ||rho_{k,k+1}(X_i) - rho_{k,k+1}(Y_j)||_F^2) = exp(-g/4 sum_k sum_pq (T(X_i)[k,p,q] - T(Y_j)[k,p,q])^2),
    T[k, p, q] = <P_p on qubit k, P_q on qubit k+1>, P = (I, X, Y, Z), k = 0 .. n_qubits - 2: 16 (n - 1) reals per state are
    all-gathered instead of 3 n.  It needs at least two qubits.

    ``pair_distance=D`` (with ``rdm=2``, 1 <= D <= n_qubits - 1) compares every pair (k, k+d), d = 1 .. D, in the order of
    ``engine.pair_table(n_qubits, D)``: for an ansatz whose entanglement map reaches distance D these are the pairs its gates
    touch (D = max(abs(a - b)) over the map).  16 n_pairs reals per state are all-gathered, n_pairs = D n - D (D + 1) / 2, and
    ``pqk_gamma=None`` means g = 1 / (n_qubits D).

    ``observables=[...]`` (Pauli strings, anything ``engine.pauli_strings(n_qubits, ...)`` takes) is the kernel on chosen observables,
        K[j, i] = exp(-g sum_m (<O_m>(X_i) - <O_m>(Y_j))^2),
    with ``pqk_gamma=None`` meaning g = 1 / len(observables): m reals per state are all-gathered.  It excludes ``rdm`` and
    ``pair_distance`` (leave them at 1).

    ``shots=S`` (with ``rdm=1`` or ``rdm=2``, any ``pair_distance``) is the kernel at S measurement shots per state instead of exact
    expectation values: each rank samples its share in the random bases ``engine.random_bases(S, n_qubits, shot_seed)`` with
    ``Context.sample(..., seed=shot_seed, first_state=<the share's offset>)`` (the states of Y are indexed after those of X) and
    estimates the Bloch vectors (``engine.estimate_paulis``) or the correlators (``engine.estimate_pair_paulis``) from the bits; the
    rest of the route is the same, and K is the same bits for any number of ranks.  ``shots=None`` is the exact kernel.
    ``observables`` together with ``shots`` is a ``ValueError``.

    ``observables=[Mpo, ...]`` (``engine.Mpo``: sums of operator strings such as a Hamiltonian, its square or a Hamming-weight
    read-out) takes the real parts of ``Context.mpo_expectations`` as the feature columns of the same kernel.  A list that mixes
    ``Mpo`` and Pauli strings is a ``ValueError``, and so are MPOs together with ``shots``.

    ``rdm=k, window=True`` for 3 <= k <= min(6, n_qubits) is the window form, the k-qubit member of the series:
        K_k[j, i] = exp(-g sum_a ||rho_{a,k}(X_i) - rho_{a,k}(Y_j)||_F^2),   a = 0 .. n_qubits - k,
    rho_{a,k} = the reduced density matrix of the qubits a .. a+k-1 (``Context.window_rdms``).  Each rank takes the window RDMs of
    its share; 2 (n - k + 1) 4^k reals per state are all-gathered and rank 0 calls ``Context.projected_window_gram``.  K is the
    same bits for any number of ranks; ``pqk_gamma=None`` means g = 1 / n_qubits.  It takes neither ``pair_distance`` other than
    1, nor ``shots``, nor ``observables`` (each a ``ValueError``): finite-shot window RDMs are out of scope.  ``window`` is the
    switch of this form: ``rdm >= 3`` without it stays the ``ValueError`` it has always been, and ``window=True`` with ``rdm`` 1 or 2
    is one too (those two keep their own routes).

    ``initial_states`` / ``initial_states_Y`` as in ``build_kernel_matrix``: the circuits are applied to given states."""
    strings = mpos = None
    if not isinstance(window, (bool, np.bool_)):
        raise ValueError(f"window must be True or False (got {window!r})")
    window = bool(window)
    if window:
        if isinstance(rdm, bool) or not isinstance(rdm, (int, np.integer)) or rdm < 3:
            raise ValueError(f"window=True is the form of rdm = 3 .. min({_engine.WINDOW_MAX_WIDTH}, n_qubits), got rdm={rdm!r} (rdm=1 and rdm=2 take no window)")
        if observables is not None:
            raise ValueError(f"observables chooses the features itself: it cannot be combined with rdm={rdm!r}")
        if shots is not None:
            raise ValueError(f"shots with rdm={rdm!r} is not supported: finite-shot window RDMs are out of scope (sample with rdm=1 or rdm=2)")
        if pair_distance != 1:
            raise ValueError(f"pair_distance={pair_distance!r} needs rdm=2: rdm={rdm!r} compares contiguous windows (leave pair_distance at 1)")
        if rdm > min(_engine.WINDOW_MAX_WIDTH, int(ansatz.num_qubits)):
            raise ValueError(f"rdm with window=True must be in 3 .. min({_engine.WINDOW_MAX_WIDTH}, n_qubits) = {min(_engine.WINDOW_MAX_WIDTH, int(ansatz.num_qubits))}, got {rdm!r}")
        rdm = int(rdm)
    if shots is not None:
        if observables is not None:
            raise ValueError("shots together with observables is not supported: sample with rdm=1 or rdm=2")
        if isinstance(shots, bool) or not isinstance(shots, (int, np.integer)) or shots < 1:
            raise ValueError(f"shots must be None or an int >= 1 (got {shots!r})")
        shots = int(shots)
    if observables is not None:
        if rdm != 1 or pair_distance != 1:
            raise ValueError(f"observables chooses the features itself: leave rdm and pair_distance at 1 (got rdm={rdm!r}, pair_distance={pair_distance!r})")
        obs = list(observables) if isinstance(observables, (list, tuple)) else observables
        n_mpo = sum(isinstance(o, _engine.Mpo) for o in obs) if isinstance(obs, list) else 0
        if n_mpo and n_mpo != len(obs):
            raise ValueError("observables mixes Mpo and Pauli strings: give a list of one kind")
        if n_mpo:
            mpos = _engine._mpo_list(obs, int(ansatz.num_qubits))  # ValueError: an Mpo of another length
        else:
            strings = _engine.pauli_strings(int(ansatz.num_qubits), observables)  # ValueError: empty list, bad spec
    n_obs = len(mpos) if mpos is not None else len(strings) if strings is not None else 0
    if not window and rdm not in (1, 2):
        raise ValueError(f"rdm must be 1 (one-qubit reduced density matrices), 2 (pairs) or, with window=True, 3 .. 6 (windows of that many qubits), got {rdm!r}")
    if rdm == 2 and int(ansatz.num_qubits) < 2:
        raise ValueError("rdm=2 compares reduced density matrices of neighbouring qubit pairs: the ansatz needs at least 2 qubits")
    if isinstance(pair_distance, bool) or not isinstance(pair_distance, (int, np.integer)):
        raise ValueError(f"pair_distance must be an int (the largest distance between the two qubits of a pair), got {pair_distance!r}")
    if pair_distance < 1 or pair_distance > max(1, int(ansatz.num_qubits) - 1):
        raise ValueError(f"pair_distance must be in 1 .. n_qubits - 1 = {int(ansatz.num_qubits) - 1}, got {pair_distance!r}")
    if rdm == 1 and pair_distance != 1:
        raise ValueError(f"pair_distance={pair_distance!r} needs rdm=2: the one-qubit form has no pairs")
    pair_distance = int(pair_distance)
    X, Y, fidelity = _checked_points(X, Y, truncation_error)
    if pqk_gamma is not None:
        _engine.projected_gamma(pqk_gamma, 1)  # ValueError unless > 0 and finite
    inits = _initial_pair(initial_states, initial_states_Y, X, Y, ansatz)
    run = _start(mpi_comm, "the projected kernel has")
    ctx = run.ctx
    n_qubits = int(ansatz.num_qubits)
    n_pairs = pair_distance * n_qubits - pair_distance * (pair_distance + 1) // 2  # n_qubits - 1 at distance 1
    prof = _profile_head(run, X, Y)
    f_shape = (n_obs,) if n_obs else (n_qubits, 3) if rdm == 1 else (n_pairs, 4, 4)
    if window:
        f_shape = (n_qubits - rdm + 1, 1 << rdm, 1 << rdm, 2)

    def features_of(label, local, lo):
        if window:  # complex128 as (re, im) pairs of float64: the features travel as the other forms' do
            return np.ascontiguousarray(ctx.window_rdms(local, rdm)).view(np.float64).reshape((len(local),) + f_shape)
        if mpos is not None:  # the real parts are the feature columns
            return np.ascontiguousarray(ctx.mpo_expectations(local, mpos).real)
        if strings is not None:
            return ctx.pauli_expectations(local, strings)
        if shots is not None:
            shot_bases = _engine.random_bases(shots, n_qubits, shot_seed)
            bits = ctx.sample(local, shots, bases=shot_bases, seed=shot_seed, first_state=int(lo) + (0 if label == "X" else len(X)))
            return _engine.estimate_paulis(bits, shot_bases)[0] if rdm == 1 else _engine.estimate_pair_paulis(bits, shot_bases, pair_distance)
        return ctx.local_paulis(local) if rdm == 1 else ctx.local_pair_paulis(local, max_dist=pair_distance)

    feats, chi_all, sim_secs, fids, feat_secs, gather_secs = _gathered_features(run, mpi_comm, ansatz, X, Y, fidelity, f_shape, features_of, inits)
    if not run.is_root:
        return None
    g = _engine.projected_gamma(pqk_gamma, n_obs if n_obs else n_qubits * pair_distance)  # (a window form has pair_distance 1)
    _say(True, "\nFinished contracting all MPS.\n\nCalculating projected kernel matrix...")
    t0 = time.perf_counter()
    if window:
        rdms = [np.ascontiguousarray(f).view(np.complex128)[..., 0] for f in feats]
        kernel_mat = ctx.projected_window_gram(rdms[0], None if Y is None else rdms[1], g)
    elif n_obs:
        kernel_mat = ctx.feature_gram(feats[0], None if Y is None else feats[1], g)
    elif rdm == 1:
        kernel_mat = ctx.projected_gram(feats[0], None if Y is None else feats[1], g)
    else:
        kernel_mat = ctx.projected_pair_gram(feats[0], None if Y is None else feats[1], g, max_dist=pair_distance)
    tiles = time.perf_counter() - t0

    prof["r0_circ_gen"] = [0.0, "seconds"]
    prof.update(_sim_stats(sim_secs))
    prof["avg_fidelity"] = [sum(fids) / max(1, len(fids)), ""]
    prof.update(_chi_stats(chi_all))
    prof["r0_RR_recv"] = [gather_secs, "seconds"]  # the all-gather of the Bloch vectors
    prof["pqk_gamma"] = [g, ""]
    if n_obs:
        prof["pqk_observables"] = [n_obs, "MPOs" if mpos is not None else "strings"]
    else:
        prof["pqk_rdm"] = [rdm, "qubits"]
    if rdm == 2:
        prof["pqk_pair_distance"] = [pair_distance, "sites"]
    if shots is not None:
        prof["pqk_shots"] = [shots, "shots"]
    prof["pqk_features_time"] = [feat_secs, "seconds"]
    prof["kernel_mat_time"] = [tiles, "seconds"]
    prof["total_time"] = [time.perf_counter() - run.t_start, "seconds"]
    _write_profile(info_file, prof)
    return kernel_mat


def build_shot_feature_kernel_matrix(mpi_comm, ansatz, X, Y=None, observables=None, window=None, shots=None, shot_seed=0, settings="random", pqk_gamma=None,
                                     truncation_error=None, info_file=None, loglevel=30):
    """The projected kernel on chosen observables or on windows of k qubits at ``shots`` measurement shots per state -- the
    finite-shot counterpart of ``build_projected_kernel_matrix(observables=...)`` and of its ``rdm=k, window=True`` form.  Exactly
    one of the two forms is given:

    ``observables=[...]`` (anything ``engine.pauli_strings(n_qubits, ...)`` takes):
        K[j, i] = exp(-g sum_m (O_hat_m(X_i) - O_hat_m(Y_j))^2),
    O_hat_m = the mean sign of the shots whose bases equal string m on its support (``Context.estimate_pauli_strings``; 0.0 where
    no shot does), ``pqk_gamma=None`` meaning g = 1 / len(observables).

    ``window=k`` (an int in 1 .. min(6, n_qubits)):
        K_k[j, i] = exp(-g sum_a ||rho_hat_{a,k}(X_i) - rho_hat_{a,k}(Y_j)||_F^2),   a = 0 .. n_qubits - k,
    rho_hat = the window RDMs rebuilt from the estimated coefficients of their 4^k strings (``Context.estimate_window_rdms``:
    Hermitian with trace 1, not positive in general), ``pqk_gamma=None`` meaning g = 1 / n_qubits.

    ``settings="random"`` measures in ``engine.random_bases(shots, n_qubits, shot_seed)``; ``settings="window"`` (with ``window``
    only) in the designed bases ``engine.window_settings(shots, n_qubits, window)``, in which a string of weight v on a window is
    seen by shots / 3^v shots; it needs ``shots >= 3^window``.  Each rank builds its share of the states, samples it with
    ``Context.sample(..., seed=shot_seed, first_state=<the share's offset>)`` (the states of Y are indexed after those of X, as in
    ``build_projected_kernel_matrix``), estimates on its device, and the values are all-gathered; rank 0 calls
    ``Context.feature_gram`` or ``Context.projected_window_gram`` and returns the ``len(Y) x len(X)`` matrix, the other ranks
    ``None``.  The estimates are ratios of integers, so K is the same bits for any number of ranks."""
    if (observables is None) == (window is None):
        raise ValueError("give exactly one of observables (a list of Pauli strings) and window (the qubits of a window)")
    n_qubits = int(ansatz.num_qubits)
    if isinstance(shots, bool) or not isinstance(shots, (int, np.integer)) or shots < 1:
        raise ValueError(f"shots must be an int >= 1 (got {shots!r})")
    shots = int(shots)
    if settings not in ("random", "window"):
        raise ValueError(f"settings must be 'random' or 'window' (got {settings!r})")
    strings = None
    if observables is not None:
        if settings == "window":
            raise ValueError("settings='window' designs the bases for the windows of window=k: it cannot be combined with observables")
        strings = _engine.pauli_strings(n_qubits, observables)  # ValueError: empty list, bad spec
    else:
        if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or not 1 <= window <= min(_engine.WINDOW_MAX_WIDTH, n_qubits):
            raise ValueError(f"window must be an int in 1 .. min({_engine.WINDOW_MAX_WIDTH}, n_qubits) = {min(_engine.WINDOW_MAX_WIDTH, n_qubits)}, got {window!r}")
        window = int(window)
        if settings == "window" and shots < 3 ** window:
            raise ValueError(f"settings='window' needs shots >= 3^window = {3 ** window} (got {shots})")
    X, Y, fidelity = _checked_points(X, Y, truncation_error)
    if pqk_gamma is not None:
        _engine.projected_gamma(pqk_gamma, 1)  # ValueError unless > 0 and finite
    run = _start(mpi_comm, "the shot-feature kernel has")
    ctx = run.ctx
    prof = _profile_head(run, X, Y)
    shot_bases = _engine.window_settings(shots, n_qubits, window) if settings == "window" else _engine.random_bases(shots, n_qubits, shot_seed)
    n_windows = 0 if strings is not None else n_qubits - window + 1
    f_shape = (len(strings),) if strings is not None else (n_windows, 1 << window, 1 << window, 2)

    def features_of(label, local, lo):
        bits = ctx.sample(local, shots, bases=shot_bases, seed=shot_seed, first_state=int(lo) + (0 if label == "X" else len(X)))
        if strings is not None:
            return ctx.estimate_pauli_strings(bits, shot_bases, strings)[0]
        # complex128 as (re, im) pairs of float64: the features travel as the other forms' do
        return np.ascontiguousarray(ctx.estimate_window_rdms(bits, shot_bases, window)[0]).view(np.float64).reshape((len(local),) + f_shape)

    feats, chi_all, sim_secs, fids, feat_secs, gather_secs = _gathered_features(run, mpi_comm, ansatz, X, Y, fidelity, f_shape, features_of)
    if not run.is_root:
        return None
    g = _engine.projected_gamma(pqk_gamma, len(strings) if strings is not None else n_qubits)
    _say(True, "\nFinished contracting all MPS.\n\nCalculating the shot-feature kernel matrix...")
    t0 = time.perf_counter()
    if strings is not None:
        kernel_mat = ctx.feature_gram(feats[0], None if Y is None else feats[1], g)
    else:
        rdms = [np.ascontiguousarray(f).view(np.complex128)[..., 0] for f in feats]
        kernel_mat = ctx.projected_window_gram(rdms[0], None if Y is None else rdms[1], g)
    tiles = time.perf_counter() - t0

    prof["r0_circ_gen"] = [0.0, "seconds"]
    prof.update(_sim_stats(sim_secs, quartiles=False))
    prof["avg_fidelity"] = [sum(fids) / max(1, len(fids)), ""]
    prof.update(_chi_stats(chi_all))
    prof["r0_RR_recv"] = [gather_secs, "seconds"]  # the all-gather of the estimates
    prof["pqk_gamma"] = [g, ""]
    if strings is not None:
        prof["pqk_observables"] = [len(strings), "strings"]
    else:
        prof["pqk_rdm"] = [window, "qubits"]
    prof["pqk_shots"] = [shots, "shots"]
    prof["pqk_settings"] = [settings, ""]
    prof["pqk_features_time"] = [feat_secs, "seconds"]
    prof["kernel_mat_time"] = [tiles, "seconds"]
    prof["total_time"] = [time.perf_counter() - run.t_start, "seconds"]
    _write_profile(info_file, prof)
    return kernel_mat


def build_entanglement_profile(mpi_comm, ansatz, X, truncation_error=None, max_values=None, info_file=None, loglevel=30):
    """Entanglement across every bond of the states of ``X``, from the same states as ``build_projected_kernel_matrix``: each rank
    builds its share (same builders, same ``QK_BUILDER`` rules), takes the Schmidt weights and purities of every bond on its
    device (``Context.bond_spectra``, ``Context.bond_purities``) and all-gathers (n - 1) m reals per state, never an MPS.
    ``max_values=m`` keeps the m largest weights of a bond; the default is the largest bond of the whole data set (agreed across
    ranks), so that every weight is there.  Every rank returns the dict
        spectra    (len(X), n - 1, m)   descending Schmidt weights of bond k (between qubits k and k+1), zero-filled
        purities   (len(X), n - 1)      sum of their squares
        norms      (len(X),)            <psi|psi>
        bond_dims  (len(X), n + 1)      true bond dimensions
    ``engine.bond_entropies``, ``engine.cap_cost`` and ``engine.schmidt_rank`` read ``spectra``."""
    X, _, fidelity = _checked_points(X, None, truncation_error)
    if max_values is not None and (isinstance(max_values, bool) or not isinstance(max_values, (int, np.integer)) or max_values < 1):
        raise ValueError(f"max_values must be an int >= 1 or None (every weight), got {max_values!r}")
    run = _start(mpi_comm, "the entanglement profile has")
    ctx, n_qubits = run.ctx, int(ansatz.num_qubits)
    # (not ``_share_features``: the ranks agree on m between the build and the features, empty shares included, and there are four arrays)
    (_, _, lo, local, sim_secs, fids), = _build_shares(run, ansatz, X, None, fidelity)
    try:
        dims = np.zeros((0, n_qubits + 1), dtype=np.float64) if local is None else np.asarray(local.dims, dtype=np.float64)
        widest = int(dims[:, 1:n_qubits].max()) if dims.size and n_qubits > 1 else 1
        m = int(max_values) if max_values is not None else max(int(w) for w in comm_allgather(mpi_comm, widest))
        t0 = time.perf_counter()
        if local is None:
            spectra, purities, norms = np.zeros((0, n_qubits - 1, m)), np.zeros((0, n_qubits - 1)), np.zeros(0)
        else:
            spectra, norms = ctx.bond_spectra(local, max_values=m, norms=True)
            purities = ctx.bond_purities(local)
    finally:
        _close_all([local])
    feat_secs = time.perf_counter() - t0
    t0 = time.perf_counter()
    out = {"spectra": _gather_features(mpi_comm, lo, spectra, len(X)), "purities": _gather_features(mpi_comm, lo, purities, len(X)),
           "norms": _gather_features(mpi_comm, lo, norms, len(X)), "bond_dims": _gather_features(mpi_comm, lo, dims, len(X)).astype(np.int32)}
    gather_secs = time.perf_counter() - t0
    if run.is_root:
        _write_profile(info_file, {"n_procs": [run.n_procs, "gpus"], "lenX": [len(X), "entries"], "r0_circ_gen": [0.0, "seconds"], "r0_circ_sim": [sum(sim_secs), "seconds"],
                                   "avg_fidelity": [sum(fids) / max(1, len(fids)), ""], "r0_RR_recv": [gather_secs, "seconds"], "pqk_bond_values": [m, "weights"],
                                   "pqk_entanglement_time": [feat_secs, "seconds"], "total_time": [time.perf_counter() - run.t_start, "seconds"]})
    return out


def build_outcome_likelihoods(mpi_comm, ansatz, X, bits, bases=None, per_state=False, truncation_error=None):
    """Log likelihoods of given outcome strings under the states of ``X`` -- shots measured on hardware, or any list of strings:
    ``logp[i, j] = log(|<b_j| U_bases |psi(x_i)>|^2 / <psi|psi>)``.  Each rank builds its share of the states (same builders, same
    ``QK_BUILDER`` rules as ``build_projected_kernel_matrix``), computes the log likelihoods of its states on its device
    (``Context.amplitudes(..., logp=True)``) and the rows are all-gathered, never an MPS.  ``bits`` is (n_strings, n_qubits) of
    0 / 1, shared by every state -- the cross table "state x string" --, or with ``per_state=True`` (len(X), n_strings, n_qubits),
    the strings of state i under state i; ``bases`` is anything ``engine.bases_table`` takes, shared by every state.  Rank 0
    returns float64 (len(X), n_strings), the other ranks ``None``; a row is the same bits for any number of ranks.
    ``engine.xeb_fidelity`` reads the result."""
    X, _, fidelity = _checked_points(X, None, truncation_error)
    n_qubits = int(ansatz.num_qubits)
    bits = np.asarray(bits)
    want = (len(X), n_qubits) if per_state else (n_qubits,)
    if bits.dtype.kind not in "iub" or bits.ndim != len(want) + 1 or bits.shape[-1] != n_qubits or (per_state and bits.shape[0] != len(X)) or bits.shape[-2] < 1:
        shape = f"({len(X)}, n_strings, {n_qubits})" if per_state else f"(n_strings, {n_qubits})"
        raise ValueError(f"bits must be an integer array of shape {shape} with n_strings >= 1; got shape {bits.shape}, dtype {bits.dtype}")
    n_strings = bits.shape[-2]
    B = None if bases is None else _engine.bases_table(bases, n_strings, n_qubits)
    run = _start(mpi_comm, "outcome likelihoods have")

    def features_of(local, lo):
        return run.ctx.amplitudes(local, bits[lo : lo + len(local)] if per_state else bits, bases=B, per_state=per_state, logp=True)[1]

    lp, lo = _share_features(run, ansatz, X, "X", fidelity, (n_strings,), features_of)[:2]
    out = _gather_features(mpi_comm, lo, lp, len(X))
    return out if run.is_root else None


def build_outcome_marginals(mpi_comm, ansatz, X, bits, bases, truncation_error=None):
    """Probabilities of partial outcomes under the states of ``X`` -- hardware shots read out on a subset of the qubits, in any
    bases, the other qubits traced out: ``p[i, j] = <psi(x_i)| prod_k P_k |psi(x_i)> / <psi|psi>`` with ``P_k`` the projector of
    bit ``bits[j, k]`` in the basis ``bases[j, k]`` on every measured qubit.  Each rank builds its share of the states (same
    builders, same ``QK_BUILDER`` rules as ``build_projected_kernel_matrix``), computes the marginals of its states on its device
    (``Context.marginals``) and the rows are all-gathered, never an MPS.  ``bits`` is (n_strings, n_qubits) of 0 / 1, ``bases``
    (n_strings, n_qubits) or one shared row of codes 0..3 (0 = not measured, 1, 2, 3 = X, Y, Z), both shared by every state.  Rank
    0 returns float64 (len(X), n_strings), the other ranks ``None``; a row is the same bits for any number of ranks.  The values
    are not clipped: a probability of exactly 0 may come out as rounding noise of either sign."""
    X, _, fidelity = _checked_points(X, None, truncation_error)
    table, codes = _engine.marginal_strings(bits, bases, int(ansatz.num_qubits))  # raises ValueError that names bits or bases
    run = _start(mpi_comm, "outcome marginals have")
    p, lo = _share_features(run, ansatz, X, "X", fidelity, (codes.shape[0],),
                            lambda local, lo: np.ascontiguousarray(run.ctx.operator_expectations(local, codes, ops=table).real))[:2]
    out = _gather_features(mpi_comm, lo, p, len(X))
    return out if run.is_root else None


def build_mpo_expectations(mpi_comm, ansatz, X, mpos, truncation_error=None):
    """Expectation values of matrix-product operators under the states of ``X``: ``v[i, m] = <psi(x_i)| H_m |psi(x_i)> / <psi|psi>``
    for a list of ``engine.Mpo`` shared by every state.  Each rank builds its share of the states (same builders, same
    ``QK_BUILDER`` rules as ``build_projected_kernel_matrix``), evaluates the MPOs on its device (``Context.mpo_expectations``) and
    the rows are all-gathered as (re, im) pairs, never an MPS.  Rank 0 returns complex128 (len(X), n_mpos), the other ranks
    ``None``; a row is the same bits for any number of ranks."""
    X, _, fidelity = _checked_points(X, None, truncation_error)
    ms = _engine._mpo_list(mpos, int(ansatz.num_qubits))  # raises ValueError that names the entry
    run = _start(mpi_comm, "MPO observables have")
    v, lo = _share_features(run, ansatz, X, "X", fidelity, (len(ms), 2),
                            lambda local, lo: np.ascontiguousarray(run.ctx.mpo_expectations(local, ms)).view(np.float64).reshape(len(local), len(ms), 2))[:2]
    out = _gather_features(mpi_comm, lo, v, len(X))
    return np.ascontiguousarray(out).view(np.complex128)[..., 0] if run.is_root else None


def build_capped_kernel_matrices(mpi_comm, ansatz, X, Y=None, caps=(16, 32, 64), max_discard=0.0, truncation_error=None, info_file=None, loglevel=30):
    """The Gram ``K`` of ``build_kernel_matrix`` and, from the SAME states, the Gram under each bond cap of ``caps``: one build, then
    per cap every rank compresses its share on its device (``Context.compress``: one canonical truncation sweep per state, at
    most ``max_discard`` of the weight dropped per bond besides the cap), the compressed shares are exchanged like the full ones
    and the Gram is swept again.  Rank 0 returns the dict
        K          (len(Y), len(X))                 the Gram of the states as built
        K_capped   {cap: (len(Y), len(X))}          the Gram of the states compressed to the cap
        fidelity   {cap: (len(X) [+ len(Y)],)}      |<psi|psi'>|^2 of every state and its compressed twin, X first
        bond_dims  {cap: (len(X) [+ len(Y)], n+1)}  the new bond table
    and the other ranks ``None``.  |K_capped - K| is bounded absolutely, not relatively: for normalised states by d (2 + d), d =
    delta_i + delta_j + delta_i delta_j, delta = sqrt(2 - 2 sqrt(fidelity))."""
    X, Y, fidelity = _checked_points(X, Y, truncation_error)
    caps = [c for c in caps]
    if not caps or any(isinstance(c, bool) or not isinstance(c, (int, np.integer)) or c < 1 for c in caps) or len(set(caps)) != len(caps):
        raise ValueError(f"caps must be distinct ints >= 1, got {caps!r}")
    if not (float(max_discard) >= 0.0 and np.isfinite(float(max_discard))):
        raise ValueError(f"max_discard must be >= 0 and finite, got {max_discard!r}")
    run = _start(mpi_comm, "the Gram path has")
    ctx, n_qubits = run.ctx, int(ansatz.num_qubits)
    shares = _build_shares(run, ansatz, X, Y, fidelity)
    build_secs = time.perf_counter() - run.t_start

    def gram_of(local_sets):
        with _exchanged(run, mpi_comm, local_sets, shares) as full:
            return _gram_of(run, mpi_comm, full)[0]

    locals_ = [s.local for s in shares]
    out = {"K": None, "K_capped": {}, "fidelity": {}, "bond_dims": {}}
    secs = {}
    try:
        out["K"] = gram_of(locals_)
        for cap in caps:
            t0 = time.perf_counter()
            small, fids, dims = [], [], []
            try:
                for s in shares:
                    if s.local is None:
                        small.append(None)
                        fid_s, dims_s = np.zeros(0), np.zeros((0, n_qubits + 1))
                    else:
                        cs, info = ctx.compress(s.local, max_bond=int(cap), max_discard=float(max_discard), info=True)
                        small.append(cs)
                        fid_s, dims_s = info["fidelity"], info["bond_dims"].astype(np.float64)
                    fids.append(_gather_features(mpi_comm, s.lo, fid_s, s.total))
                    dims.append(_gather_features(mpi_comm, s.lo, dims_s, s.total))
                secs[cap] = time.perf_counter() - t0
                out["K_capped"][cap] = gram_of(small)
            finally:
                _close_all(small)
            out["fidelity"][cap] = np.concatenate(fids)
            out["bond_dims"][cap] = np.concatenate(dims).astype(np.int32)
    finally:
        _close_all(locals_)
    if not run.is_root:
        return None
    _write_profile(info_file, {**_profile_head(run, X, Y), "r0_circ_sim": [build_secs, "seconds"], "caps": [[int(c) for c in caps], "chi"],
                               "r0_compress": [[secs[c] for c in caps], "seconds"], "min_fidelity": [[float(out["fidelity"][c].min()) for c in caps], ""],
                               "total_time": [time.perf_counter() - run.t_start, "seconds"]})
    return out


def build_symmetrized_kernel_matrix(mpi_comm, ansatz, X, Y=None, projector=None, truncation_error=None, max_bond=None, min_weight=1e-12):
    """The fidelity kernel of the feature states projected by an MPO ``P`` (``engine.Mpo``, for instance
    ``engine.mpo_parity_projector``):
        K[j][i] = |<psi(y_j)| P^dagger P |psi(x_i)>|^2 / (w(x_i) w(y_j)),      w(x) = <psi(x)| P^dagger P |psi(x)>
    Each rank builds its share of the states (the builders of ``build_kernel_matrix``), applies ``P`` to it on its device
    (``Context.apply_mpo``) and compresses the product with ``max_discard = 0`` (only rank-deficient bonds shrink) and the cap
    ``max_bond`` (``None``: no cap), as ``build_capped_kernel_matrices`` compresses its shares; ``truncation_error`` is the
    builder's, as in ``build_kernel_matrix``.  The projected shares are exchanged and swept like the plain ones.  The weights ``w`` are the squared norms of the exact product
    states themselves.  A data point with ``w <= min_weight`` (a state outside the sector) is a ``ValueError`` that names it, on
    every rank, before anything is compressed.  Rank 0 returns ``K`` (len(Y or X), len(X)), the other ranks ``None``; any number
    of ranks gives the same bits."""
    if not isinstance(projector, _engine.Mpo):
        raise ValueError(f"projector must be an engine.Mpo, got {type(projector).__name__}")
    n_qubits = int(ansatz.num_qubits)
    if projector.n_sites != n_qubits:
        raise ValueError(f"the projector has {projector.n_sites} sites, the ansatz has {n_qubits} qubits")
    X, Y, fidelity = _checked_points(X, Y, truncation_error)
    if not (float(min_weight) >= 0.0 and np.isfinite(float(min_weight))):
        raise ValueError(f"min_weight must be >= 0 and finite, got {min_weight!r}")
    run = _start(mpi_comm, "the Gram path has")
    ctx = run.ctx
    shares, prods, small, weights = [], [], [], []  # per data set: the share, its exact product or None, the compressed twin, the weights of the whole set
    try:
        for xs, ys in ((X, None), (None, Y)) if Y is not None else ((X, None),):  # one data set at a time: the share of X is closed before Y is built
            shares += _build_shares(run, ansatz, xs, ys, fidelity)
            s = shares[-1]
            try:
                prods.append(None if s.local is None else ctx.apply_mpo(s.local, projector))
            finally:
                _close_all([s.local])
            w = np.zeros(0) if prods[-1] is None else ctx.local_paulis(prods[-1], norms=True)[1]
            weights.append(_gather_features(mpi_comm, s.lo, w, s.total))
        for s, w in zip(shares, weights):
            bad = np.flatnonzero(~(w > float(min_weight)))
            if bad.size:
                raise ValueError(f"data point {int(bad[0])} of {s.label} has weight {w[bad[0]]:.3e} <= min_weight = {float(min_weight):.3e} in the projector's sector")
        for prod in prods:
            small.append(None if prod is None else ctx.compress(prod, max_bond=max_bond, max_discard=0.0))
        with _exchanged(run, mpi_comm, small, shares) as full:
            K, _ = _gram_of(run, mpi_comm, full)
    finally:
        _close_all(prods + small)
    if not run.is_root:
        return None
    return K / np.outer(weights[-1], weights[0])


def _shot_block_share(mpi_comm, ctx, shares, n_qubits, n_procs, rank, widths, side, shots, shot_seed):
    """The finite-shot route of ``build_block_kernel_matrices``: (parts, self_x, self_y, err_x, err_y) with parts the all-gathered
    (pairs, estimates, standard errors) of every rank.  Each rank samples its share of the states, the packed words of the block (4
    bytes per shot) and the bond tables are all-gathered, and each rank estimates its share of the pairs of ``Plan(orient=False)``."""
    U, M = shots
    bases = _engine.setting_bases(U, M, n_qubits, shot_seed)
    nbits = min(n_qubits, _engine.SHOT_BLOCK_MAX_WIDTH)
    tables, dims, first = [], [], 0
    for _, total, lo, loc, _, _ in shares:  # X, then Y: the states of Y are indexed after those of X
        if loc is None:
            words, d = np.zeros((0, U * M), dtype=np.uint32), np.zeros((0, n_qubits + 1), dtype=np.int32)
        else:
            bits = ctx.sample(loc, U * M, bases=bases, seed=shot_seed, first_state=first + int(lo))
            words, d = _engine.pack_block_words(bits, side), np.asarray(loc.dims, dtype=np.int32)
        full_w, full_d = np.zeros((total, U * M), dtype=np.uint32), np.zeros((total, n_qubits + 1), dtype=np.int32)
        for s_lo, s_w, s_d in comm_allgather(mpi_comm, (int(lo), words, d)):
            full_w[s_lo : s_lo + len(s_w)], full_d[s_lo : s_lo + len(s_d)] = s_w, s_d
        # the words as outcome tables of the block alone: bit k of a word is qubit k of a left block
        tables.append(np.ascontiguousarray(((full_w[..., None] >> np.arange(nbits, dtype=np.uint32)) & np.uint32(1)).astype(np.uint8)))
        dims.append(full_d)
        first += total
    bx, by = tables[0], tables[1] if len(tables) > 1 else None
    plan = _engine.Plan(dims[0], None if by is None else dims[1], n_procs, rank, orient=False)
    try:
        pairs = plan.pairs()
    finally:
        plan.close()
    if len(pairs):
        sums, S = ctx.shot_block_sums_host(bx, by, U, pairs, widths, "left", per_setting=True)
        vals, errs = _engine.shot_block_estimate(sums, S, U, M, (pairs[:, 0] == pairs[:, 1]) if by is None else False)
    else:
        vals = errs = np.zeros((len(widths), 0))
    parts = comm_allgather(mpi_comm, (pairs, vals, errs))

    def self_of(b):
        d = np.arange(b.shape[0])
        sums, S = ctx.shot_block_sums_host(b, None, U, np.stack([d, d], axis=1), widths, "left", per_setting=True)
        return _engine.shot_block_estimate(sums, S, U, M, True)

    if by is None:
        return parts, None, None, None, None
    (self_x, err_x), (self_y, err_y) = self_of(bx), self_of(by)
    return parts, self_x, self_y, err_x, err_y


def build_block_kernel_matrices(mpi_comm, ansatz, X, Y=None, widths=None, side="left", form="rbf", block_gamma=None, truncation_error=None, info_file=None,
                                loglevel=30, shots=None, shot_seed=0):
    """Block kernels: from ONE build of the states, the projected kernel of the reduced state of the first (``side="left"``) or last
    (``"right"``) w qubits, for every w of ``widths`` (strictly increasing ints in 1 .. num_qubits; ``None``: every width).  One pair
    sweep gives the whole family between the one-qubit kernel (w = 1) and the fidelity kernel (w = n).  Rank 0 returns the dict
        widths    [w, ...]
        K         {w: (len(Y), len(X))}    the kernel of ``form``: "overlap", "normalized" or "rbf" (``engine.block_kernel``;
                                           ``block_gamma`` is the rbf's gamma, default 1)
        overlap   {w: (len(Y), len(X))}    O_w[j, i] = tr(rho_A(x_i) rho_A(y_j))
        self_x    (n_widths, len(X))       S_w(x_i) = tr(rho_A(x_i)^2)
        self_y    (n_widths, len(Y))       (``self_x`` when Y is None)
    and the other ranks ``None``.  The shares are built and exchanged as in ``build_capped_kernel_matrices``; each rank sweeps its
    share of the pairs (``Context.block_values_host``) and the shares meet in one all-gather on the communicator.  The self
    overlaps are linear work: every rank computes them for all states.

    ``shots=(U, M)`` is the family at finite shots, by the randomised-measurement protocol (Elben et al., PRL 124, 010504 (2020)):
    U random settings of M shots each.  Each rank samples its share in ``engine.setting_bases(U, M, num_qubits, shot_seed)`` with
    ``Context.sample(..., seed=shot_seed, first_state=<the share's offset>)`` (the states of Y are indexed after those of X), the
    packed words of the block (4 bytes per shot) are all-gathered instead of the states, and each rank estimates its share of the
    pairs of the same plan (``Context.shot_block_sums_host``, ``engine.shot_block_estimate``).  ``overlap``, ``K``, ``self_x`` and
    ``self_y`` then hold the estimates -- in a symmetric call the diagonal of ``overlap`` is the purity estimate ``self_x`` -- and the
    dict gains
        shots     (U, M)
        stderr    {"overlap": {w: (len(Y), len(X))}, "self_x": (n_widths, len(X)), "self_y": (n_widths, len(Y))}
    The sums are integers, so ``K`` is the same bits for any number of ranks.  A width above 32 together with ``shots`` is a
    ``ValueError``.  ``shots=None`` is the exact family."""
    X, Y, fidelity = _checked_points(X, Y, truncation_error)
    n_qubits = int(ansatz.num_qubits)
    if widths is None:
        widths = range(1, n_qubits + 1)
    widths = [w for w in widths]
    if (not widths or any(isinstance(w, bool) or not isinstance(w, (int, np.integer)) or not 1 <= w <= n_qubits for w in widths)
            or any(b <= a for a, b in zip(widths, widths[1:]))):
        raise ValueError(f"widths must be strictly increasing ints in 1 .. {n_qubits}, got {widths!r}")
    widths = [int(w) for w in widths]
    if side not in ("left", "right"):
        raise ValueError(f"side must be 'left' or 'right', got {side!r}")
    if form not in ("overlap", "normalized", "rbf"):
        raise ValueError(f"form must be 'overlap', 'normalized' or 'rbf', got {form!r}")
    if block_gamma is not None and not (float(block_gamma) > 0.0 and np.isfinite(float(block_gamma))):
        raise ValueError(f"block_gamma must be > 0 and finite, got {block_gamma!r}")
    if shots is not None:
        if (not isinstance(shots, (tuple, list)) or len(shots) != 2
                or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1 for v in shots)):
            raise ValueError(f"shots must be None or (settings, shots_per_setting), two ints >= 1 (got {shots!r})")
        shots = (int(shots[0]), int(shots[1]))
        if widths[-1] > _engine.SHOT_BLOCK_MAX_WIDTH:
            raise ValueError(f"shots: a packed word holds {_engine.SHOT_BLOCK_MAX_WIDTH} qubits, so widths stop there (got {widths[-1]})")
        if Y is None and shots[1] < 2:
            raise ValueError("shots: the purity estimates of a symmetric call need shots_per_setting >= 2")
    run = _start(mpi_comm, "the Gram path has")
    ctx, rank, n_procs = run.ctx, run.rank, run.n_procs
    shares = _build_shares(run, ansatz, X, Y, fidelity)
    build_secs = time.perf_counter() - run.t_start
    locals_ = [s.local for s in shares]
    prof = {**_profile_head(run, X, Y), "r0_circ_sim": [build_secs, "seconds"], "widths": [widths, "qubits"], "side": [side, ""]}
    ny = len(X) if Y is None else len(Y)
    if shots is not None:
        try:
            t0 = time.perf_counter()
            parts, self_x, self_y, err_x, err_y = _shot_block_share(mpi_comm, ctx, shares, n_qubits, n_procs, rank, widths, side, shots, shot_seed)
            sweep_secs = time.perf_counter() - t0
        finally:
            _close_all(locals_)
        if not run.is_root:
            return None
        out = {"widths": widths, "K": {}, "overlap": {}, "self_x": self_x, "self_y": self_y, "shots": shots, "stderr": {"overlap": {}, "self_x": err_x, "self_y": err_y}}
        for wi, w in enumerate(widths):
            O = assemble_gram(ny, len(X), [p[0] for p in parts], [p[1][wi] for p in parts], Y is None)
            out["overlap"][w] = O
            out["stderr"]["overlap"][w] = assemble_gram(ny, len(X), [p[0] for p in parts], [p[2][wi] for p in parts], Y is None)
        if Y is None:  # the diagonal of a symmetric call is the purity estimate
            d = np.arange(len(X))
            out["self_x"] = out["self_y"] = np.stack([out["overlap"][w][d, d] for w in widths])
            out["stderr"]["self_x"] = out["stderr"]["self_y"] = np.stack([out["stderr"]["overlap"][w][d, d] for w in widths])
        for wi, w in enumerate(widths):
            out["K"][w] = _engine.block_kernel(out["overlap"][w], out["self_x"][wi], None if Y is None else out["self_y"][wi], form=form, gamma=block_gamma)
        _write_profile(info_file, {**prof, "block_shots": [list(shots), "settings, shots"], "r0_block_sweep": [sweep_secs, "seconds"],
                                   "total_time": [time.perf_counter() - run.t_start, "seconds"]})
        return out
    try:
        with _exchanged(run, mpi_comm, locals_, shares) as full:
            xset, yset = full[0], full[1] if len(full) > 1 else None
            t0 = time.perf_counter()
            # (orient=False: a symmetric plan lists i <= j for every world size, so a value is the same bits however many ranks share the pairs)
            plan = _engine.Plan(xset.dims, None if yset is None else yset.dims, n_procs, rank, orient=False)
            try:
                vals = ctx.block_values_host(xset, yset, plan, widths, side)
                parts = comm_allgather(mpi_comm, (plan.pairs(), vals))
            finally:
                plan.close()
            self_x = ctx.block_self(xset, widths, side)
            self_y = self_x if yset is None else ctx.block_self(yset, widths, side)
            sweep_secs = time.perf_counter() - t0
    finally:
        _close_all(locals_)
    if not run.is_root:
        return None
    out = {"widths": widths, "K": {}, "overlap": {}, "self_x": self_x, "self_y": self_y}
    for wi, w in enumerate(widths):
        O = assemble_gram(ny, len(X), [p[0] for p in parts], [p[1][wi] for p in parts], Y is None)
        out["overlap"][w] = O
        out["K"][w] = _engine.block_kernel(O, self_x[wi], None if Y is None else self_y[wi], form=form, gamma=block_gamma)
    _write_profile(info_file, {**prof, "r0_block_sweep": [sweep_secs, "seconds"], "total_time": [time.perf_counter() - run.t_start, "seconds"]})
    return out


def _shadow_share(mpi_comm, ctx, shares, n_qubits, n_procs, rank, shots, shot_seed, bases):
    """The pair share of ``build_shadow_kernel_matrix``: the all-gathered (pairs, histograms, equal-shot histograms) of every rank.
    Each rank samples its share of the states, the packed records (12 bytes per 32 qubits per shot) and the bond tables are
    all-gathered, and each rank counts its share of the pairs of ``Plan(orient=False)``."""
    groups = (n_qubits + 31) // 32
    tables, dims, first = [], [], 0
    for _, total, lo, loc, _, _ in shares:  # X, then Y: the states of Y are indexed after those of X
        if loc is None:
            recs, d = np.zeros((0, shots, groups, 3), dtype=np.uint32), np.zeros((0, n_qubits + 1), dtype=np.int32)
        else:
            bits = ctx.sample(loc, shots, bases=bases, seed=shot_seed, first_state=first + int(lo))
            recs, d = _engine.pack_shadow_words(bits, bases), np.asarray(loc.dims, dtype=np.int32)
        full_r, full_d = np.zeros((total, shots, groups, 3), dtype=np.uint32), np.zeros((total, n_qubits + 1), dtype=np.int32)
        for s_lo, s_r, s_d in comm_allgather(mpi_comm, (int(lo), recs, d)):
            full_r[s_lo : s_lo + len(s_r)], full_d[s_lo : s_lo + len(s_d)] = s_r, s_d
        # plane 0 of the records back as an outcome table: bit k % 32 of group k // 32 is qubit k
        k = np.arange(n_qubits)
        tables.append(np.ascontiguousarray(((full_r[:, :, k // 32, 0] >> (k % 32).astype(np.uint32)) & np.uint32(1)).astype(np.uint8)))
        dims.append(full_d)
        first += total
    bx, by = tables[0], tables[1] if len(tables) > 1 else None
    plan = _engine.Plan(dims[0], None if by is None else dims[1], n_procs, rank, orient=False)
    try:
        pairs = plan.pairs()
    finally:
        plan.close()
    if len(pairs):
        H, E = ctx.shadow_hist_host(bx, bases, by, None if by is None else bases, pairs, equal=True)
    else:
        H = E = np.zeros((0, 2 * n_qubits + 1), dtype=np.int64)
    return comm_allgather(mpi_comm, (pairs, H, E))


def build_shadow_kernel_matrix(mpi_comm, ansatz, X, Y=None, shots=None, shot_seed=0, shadow_gamma=1.0, shadow_tau=1.0, skip_equal_shots=True, truncation_error=None,
                               info_file=None, return_hist=False):
    """The classical-shadow kernel of Huang, Kueng, Torlai, Albert and Preskill (Science 377, eabk3333 (2022)) from ``shots``
    randomised-measurement shots per state, all n qubits of every shot:
        K[j, i] = exp(shadow_tau * mean over the shot pairs (t, t') of exp(shadow_gamma / n * sum_k tr(sigma_k(x_i, t) sigma_k(y_j, t'))))
    with sigma = 3 |s><s| - I the single-qubit shadow of a shot (the paper: gamma = tau = 1).  A shot pair enters only through the
    integer d = (qubits measured in the same basis with the same outcome) - (same basis, other outcome), so the device counts the
    exact histogram of d for every pair of states (``Context.shadow_hist_host``) and the weights are applied on the host
    (``engine.shadow_kernel``): a scan over gamma and tau needs the histograms once (``return_hist=True``).

    Each rank builds its share of the states and samples it in ``engine.random_bases(shots, num_qubits, shot_seed)`` with
    ``Context.sample(..., seed=shot_seed, first_state=<the share's offset>)`` (the states of Y are indexed after those of X); the
    packed records (12 bytes per 32 qubits per shot) and the bond tables are all-gathered instead of the states, and each rank
    counts its share of the pairs of ``Plan(orient=False)``.  Rank 0 returns K of shape (len(Y), len(X)) -- (len(X), len(X)) and
    exactly symmetric when Y is None -- and with ``return_hist=True`` the tuple ``(K, {"hist": (ny, nx, 2 n + 1) int64, "equal":
    the same shape})``; the other ranks return ``None``.  The counts are integers, so K is the same bits for any number of ranks.

    Every state, of X and of Y, is measured in ONE shared bases table, because ``Context.sample`` takes one table for a whole set.
    The shot pairs with t = t' therefore share their bases on every qubit (d has the full weight of n qubits instead of about n / 3)
    and bias a cross-pair value at order 1 / shots.  ``skip_equal_shots=True`` (the default) removes exactly those ``shots`` pairs
    from every entry, leaving the mean over the shots (shots - 1) pairs with t != t'; in a self pair they are a shot paired with
    itself.  ``skip_equal_shots=False`` keeps every pair: the Gram of the inner mean is then positive semi-definite exactly (an inner
    product of mean feature vectors).  Either way the diagonal of a symmetric K is the self pair's value, an estimate like the others,
    not exactly 1 or any other constant.  ``shots`` must be an int >= 2; ``num_qubits > 128`` is a ``ValueError``."""
    X, Y, fidelity = _checked_points(X, Y, truncation_error)
    n_qubits = int(ansatz.num_qubits)
    if n_qubits > _engine.SHADOW_MAX_QUBITS:
        raise ValueError(f"the shadow kernel's records hold at most {_engine.SHADOW_MAX_QUBITS} qubits (num_qubits is {n_qubits})")
    if isinstance(shots, bool) or not isinstance(shots, (int, np.integer)) or shots < 2:
        raise ValueError(f"shots must be an int >= 2 (got {shots!r})")
    shots = int(shots)
    for name, v in (("shadow_gamma", shadow_gamma), ("shadow_tau", shadow_tau)):
        if not np.isfinite(float(v)):
            raise ValueError(f"{name} must be finite, got {v!r}")
    run = _start(mpi_comm, "the Gram path has")
    shares = _build_shares(run, ansatz, X, Y, fidelity)
    build_secs = time.perf_counter() - run.t_start
    try:
        t0 = time.perf_counter()
        parts = _shadow_share(mpi_comm, run.ctx, shares, n_qubits, run.n_procs, run.rank, shots, shot_seed, _engine.random_bases(shots, n_qubits, shot_seed))
        sweep_secs = time.perf_counter() - t0
    finally:
        _close_all(s.local for s in shares)
    if not run.is_root:
        return None
    nx, ny = len(X), len(X) if Y is None else len(Y)
    hist, equal = np.zeros((ny, nx, 2 * n_qubits + 1), dtype=np.int64), np.zeros((ny, nx, 2 * n_qubits + 1), dtype=np.int64)
    for pairs, H, E in parts:
        for dst, src in ((hist, H), (equal, E)):
            dst[pairs[:, 1], pairs[:, 0]] = src
            if Y is None:
                dst[pairs[:, 0], pairs[:, 1]] = src
    K = _engine.shadow_kernel(hist, n_qubits, shadow_gamma, shadow_tau, equal if skip_equal_shots else None)
    _write_profile(info_file, {**_profile_head(run, X, Y), "r0_circ_sim": [build_secs, "seconds"], "shadow_shots": [shots, "shots"], "r0_shadow_sweep": [sweep_secs, "seconds"],
                               "total_time": [time.perf_counter() - run.t_start, "seconds"]})
    return (K, {"hist": hist, "equal": equal}) if return_hist else K


def _depth_scan_share(ctx, ansatz, points, rank, n_procs, fidelity, depths, ends, is_root, label, host_workers):
    """This rank's slice of ``points`` (the chunks of ``_simulate_share``) at every depth of ``depths`` (ascending): (first index,
    {depth: packed device set, or None for an empty share}, {depth: fidelities}).  One launch of the device builder to the deepest
    depth with checkpoints at the layer ends; if the device gives up, one host build per depth on the sliced circuits."""
    import os

    lo, hi = _chunk(len(points), rank, n_procs)
    if hi <= lo:
        return lo, {r: None for r in depths}, {r: [] for r in depths}
    deepest = ends[depths[-1] - 1]
    circuits = [as_bound_circuit(ansatz.circuit_for_data(points[k, :]), ansatz).sliced(0, deepest) for k in range(lo, hi)]
    reject_channels(circuits, "build_depth_scan_kernel_matrices")
    chi = int(os.environ.get("QK_MAX_BOND", "0")) or None
    cap = chi or int(os.environ.get("QK_BUILDER_MAX_BOND", "320"))
    sets, fids = {}, {}
    try:
        with ctx.build_mps_scan(circuits, [ends[r - 1] for r in depths], fidelity, max_bond=cap, truncate=chi is not None) as scan:
            for j, r in enumerate(depths):
                sets[r], fids[r] = scan.set(j), [float(f) for f in scan.info(j)["fidelity"]]
    except _engine.QkError as exc:
        for m in sets.values():
            m.close()
        _say(is_root, f"{label}: device builder gave up on the depth scan ({exc}); one host build per depth")
        sets, fids = {}, {}
        for r in depths:
            states, _ = simulate_many([c.sliced(0, ends[r - 1]) for c in circuits], fidelity, workers=host_workers, max_bond=chi)
            sets[r], fids[r] = ctx.upload(states), [m.fidelity for m in states]
    _say(is_root, f"{label}: 100%")
    return lo, sets, fids


def build_depth_scan_kernel_matrices(mpi_comm, ansatz, X, Y=None, depths=(1,), truncation_error=None, info_file=None, loglevel=30):
    """The Gram of ``build_kernel_matrix`` at several depths of the ansatz from ONE build: ``depths`` are distinct layer counts in
    1 .. ``ansatz.reps``.  The ansatz repeats one layer, so the circuit of depth r is a prefix of the deeper ones: each rank builds
    its share to ``max(depths)`` in one launch of the device builder with checkpoints at the layer ends (``ansatz.layer_ends()``,
    ``Context.build_mps_scan``); per depth the shares are exchanged and swept like any set.  Rank 0 returns the dict
        depths     the depths, ascending
        K          {r: (len(Y), len(X))}            the Gram of the ansatz with r layers
        fidelity   {r: (len(X) [+ len(Y)],)}        the builder's fidelity of every state at that depth, X first
        bond_dims  {r: (len(X) [+ len(Y)], n+1)}    the bond tables
    and the other ranks ``None``.  QK_MAX_BOND (a bond cap) and QK_BUILDER_MAX_BOND (the largest bond the device builder holds,
    320) mean what they mean for ``build_kernel_matrix``'s device builder; a state that outgrows the latter, or any other device
    failure, sends the share to the host builder, one build per depth (the log says so)."""
    X, Y, fidelity = _checked_points(X, Y, truncation_error)
    depths = sorted(check_depths(depths, ansatz.reps))
    ends = [int(e) for e in ansatz.layer_ends()]
    run = _start(mpi_comm, "the Gram path has")
    shares = []  # _Share with {depth: set} for the local set and {depth: fidelities} for the fidelities
    for label, points in (("X", X), ("Y", Y)):
        if points is None:
            continue
        _say(run.is_root, f"\nContracting the MPS of the circuits from the {label} dataset at depths {depths}...")
        lo, sets, fids = _depth_scan_share(run.ctx, ansatz, points, run.rank, run.n_procs, fidelity, depths, ends, run.is_root, label, run.host_workers)
        shares.append(_Share(label, len(points), lo, sets, [], fids))
    run.ctx.trim()
    build_secs = time.perf_counter() - run.t_start
    out = {"depths": list(depths), "K": {}, "fidelity": {}, "bond_dims": {}}
    gram_secs = {}
    n_qubits = int(ansatz.num_qubits)
    try:
        for r in depths:
            t0 = time.perf_counter()
            fids, dims = [], []
            for s in shares:
                fids.append(_gather_features(mpi_comm, s.lo, np.asarray(s.fids[r], dtype=np.float64), s.total))
                d = np.zeros((0, n_qubits + 1)) if s.local[r] is None else np.asarray(s.local[r].dims, dtype=np.float64)
                dims.append(_gather_features(mpi_comm, s.lo, d, s.total))
            with _exchanged(run, mpi_comm, [s.local[r] for s in shares], shares) as full:
                out["K"][r], _ = _gram_of(run, mpi_comm, full)
            out["fidelity"][r] = np.concatenate(fids)
            out["bond_dims"][r] = np.concatenate(dims).astype(np.int32)
            gram_secs[r] = time.perf_counter() - t0
    finally:
        _close_all(m for s in shares for m in s.local.values())
    if not run.is_root:
        return None
    _write_profile(info_file, {**_profile_head(run, X, Y), "depths": [list(depths), "layers"], "r0_circ_sim": [build_secs, "seconds"],
                               "kernel_mat_time": [[gram_secs[r] for r in depths], "seconds"], "max_chi": [[int(out["bond_dims"][r].max()) for r in depths], "chi"],
                               "total_time": [time.perf_counter() - run.t_start, "seconds"]})
    return out


def _noisy_share(ansatz, points, first_index, trajectories, noise_seed, rank, n_procs, fidelity, is_root, label, device_id, initial=None):
    """This rank's slice of a data set, every point as ``trajectories`` quantum trajectories -> (first point, the states as one
    device set in the order (point, trajectory) -- ``None`` for an empty share --, the log-weights (m, T), does the ansatz hold
    channels).  Data point p of the slice's data set has state index ``first_index + p`` and its trajectories are 0 .. T-1, so the
    draws do not depend on the number of ranks.  QK_BUILDER=host builds on the host (``mps.simulate`` with the same seed and
    indices); any other value on the device, bonds up to QK_BUILDER_MAX_BOND (320) or QK_MAX_BOND (a cap), and a share the device
    gives up on is rebuilt on the host with the same seed and indices unless the device was forced.  ``initial`` (``_initial_states``)
    starts the circuits from given states: the T trajectories of a point share its one input state (``index`` of ``Context.seed``)."""
    import os

    T = int(trajectories)
    lo, hi = _chunk(len(points), rank, n_procs)
    if hi <= lo:
        return lo, None, np.zeros((0, T)), False
    circuits = [as_bound_circuit(ansatz.circuit_for_data(points[k, :]), ansatz) for k in range(lo, hi)]
    noisy = any(c.n_channel_gates > 0 for c in circuits)
    expanded = [c for c in circuits for _ in range(T)]
    sidx = np.repeat(np.arange(lo, hi, dtype=np.int64) + int(first_index), T)
    traj = np.tile(np.arange(T, dtype=np.int64), hi - lo)
    chi = int(os.environ.get("QK_MAX_BOND", "0")) or None
    which = os.environ.get("QK_BUILDER", "auto")
    ctx = _engine.default_context(device_id)
    inits = _share_of(initial, lo, hi)
    if which != "host":
        cap = chi or int(os.environ.get("QK_BUILDER_MAX_BOND", "320"))
        try:
            given = {}
            if inits is not None:  # one seed state per point (or one for all), T builds each
                given = {"initial": inits if isinstance(inits, list) else [inits],
                         "initial_index": np.repeat(np.arange(hi - lo, dtype=np.int32), T) if isinstance(inits, list) else np.zeros((hi - lo) * T, dtype=np.int32)}
            dset, info = ctx.build_mps_set(expanded, fidelity, max_bond=cap, truncate=chi is not None, seed=noise_seed, state_index=sidx, trajectory=traj, **given)
            _say(is_root, f"{label}: 100%")
            return lo, dset, np.asarray(info["logw"]).reshape(hi - lo, T), noisy
        except _engine.QkError as exc:
            if which == "device":
                raise
            _say(is_root, f"{label}: device builder gave up ({exc}); building on the host")
    per_state = [None] * len(expanded) if inits is None else [inits[k // T] if isinstance(inits, list) else inits for k in range(len(expanded))]
    states = [simulate(c, fidelity, max_bond=chi, seed=noise_seed, state_index=int(s), trajectory=int(t), initial=m) for c, s, t, m in zip(expanded, sidx, traj, per_state)]
    _say(is_root, f"{label}: 100%")
    return lo, ctx.upload(states), np.array([m.logw for m in states]).reshape(hi - lo, T), noisy


def _noisy_arguments(X, Y, trajectories, noise_seed, truncation_error):
    """The argument checks the two noisy drivers share -> (X, Y, fidelity, trajectories)."""
    X, Y, fidelity = _checked_points(X, Y, truncation_error)
    if isinstance(trajectories, bool) or not isinstance(trajectories, (int, np.integer)) or trajectories < 1:
        raise ValueError(f"trajectories must be an int >= 1 (got {trajectories!r})")
    _engine._seed_key(noise_seed)
    return X, Y, fidelity, int(trajectories)


def build_noisy_projected_kernel_matrix(mpi_comm, ansatz, X, Y=None, trajectories=1, noise_seed=0, rdm=1, pair_distance=1, pqk_gamma=None, truncation_error=None,
                                        initial_states=None, initial_states_Y=None):
    """The projected kernel of ``build_projected_kernel_matrix`` (``rdm=1`` or ``rdm=2`` with ``pair_distance``) for an ansatz with
    Kraus channels (``engine.with_noise``, the channel names of ``BoundCircuit.from_gates``): every data point is run as
    ``trajectories`` quantum trajectories and its features are the mean over them of ``local_paulis`` / ``local_pair_paulis`` -- the
    Bloch vectors / pair correlators of the trajectory-averaged state rho = mean |psi_a><psi_a|, an unbiased estimate of the noisy
    state's (the features are linear in rho: the cost is linear in T).  Then the existing Gram.  Data point p (Y after X) has state
    index p and its trajectories are 0 .. T-1 (``channel_uniform(noise_seed, gate, trajectory, p)``), so any number of ranks gives
    the same bits; ``trajectories=1`` with an ansatz without channels is ``build_projected_kernel_matrix`` to rounding.  Returns
    the ``len(Y) x len(X)`` matrix on rank 0, ``None`` elsewhere.  ``initial_states`` / ``initial_states_Y`` as in
    ``build_kernel_matrix``: every trajectory of a point starts from the point's given state."""
    if rdm not in (1, 2):
        raise ValueError(f"rdm must be 1 or 2, got {rdm!r}")
    n_qubits = int(ansatz.num_qubits)
    if isinstance(pair_distance, bool) or not isinstance(pair_distance, (int, np.integer)) or not 1 <= pair_distance <= max(1, n_qubits - 1):
        raise ValueError(f"pair_distance must be an int in 1 .. n_qubits - 1 = {n_qubits - 1}, got {pair_distance!r}")
    if rdm == 1 and pair_distance != 1:
        raise ValueError(f"pair_distance={pair_distance!r} needs rdm=2: the one-qubit form has no pairs")
    if rdm == 2 and n_qubits < 2:
        raise ValueError("rdm=2 compares reduced density matrices of qubit pairs: the ansatz needs at least 2 qubits")
    if pqk_gamma is not None:
        _engine.projected_gamma(pqk_gamma, 1)
    X, Y, fidelity, T = _noisy_arguments(X, Y, trajectories, noise_seed, truncation_error)
    pair_distance = int(pair_distance)
    run = _start(mpi_comm, "the noisy kernels have")
    ctx = run.ctx
    n_pairs = pair_distance * n_qubits - pair_distance * (pair_distance + 1) // 2
    feats = []
    inits = _initial_pair(initial_states, initial_states_Y, X, Y, ansatz)
    for label, points, first, initial in (("X", X, 0, inits[0]), ("Y", Y, len(X), inits[1])):
        if points is None:
            continue
        lo, local, _, _ = _noisy_share(ansatz, points, first, T, noise_seed, run.rank, run.n_procs, fidelity, run.is_root, label, run.device_id, initial)
        ctx.trim()
        if local is None:
            F = np.zeros((0, n_qubits, 3) if rdm == 1 else (0, n_pairs, 4, 4), dtype=np.float64)
        else:
            try:
                F = ctx.local_paulis(local) if rdm == 1 else ctx.local_pair_paulis(local, max_dist=pair_distance)
            finally:
                local.close()
            F = np.asarray(F, dtype=np.float64)
            F = F.reshape((F.shape[0] // T, T) + F.shape[1:]).mean(axis=1)  # the features of the trajectory-averaged state
        feats.append(_gather_features(mpi_comm, lo, F, len(points)))
    if not run.is_root:
        return None
    g = _engine.projected_gamma(pqk_gamma, n_qubits * pair_distance)
    if rdm == 1:
        return ctx.projected_gram(feats[0], None if Y is None else feats[1], g)
    return ctx.projected_pair_gram(feats[0], None if Y is None else feats[1], g, max_dist=pair_distance)


def build_noisy_kernel_matrix(mpi_comm, ansatz, X, Y=None, trajectories=2, noise_seed=0, truncation_error=None):
    """The fidelity kernel of noisy states from quantum trajectories: ``K[j, i] = mean_{a,b} |<psi_a(X_i)|psi_b(Y_j)>|^2``, an
    unbiased estimate of ``tr(rho(X_i) rho(Y_j))`` for rho = the trajectory-averaged state, taken from ONE fidelity Gram of the
    expanded sets (T states per point) and averaged on the host.  ``Y=None`` means ``Y = X``; on its diagonal the a = b terms (which
    are 1) are left out -- the unbiased estimate of the purity tr(rho^2) -- so a symmetric call on an ansatz with channels needs
    ``trajectories >= 2``.  State indices and trajectories as in ``build_noisy_projected_kernel_matrix``: the same bits for any
    number of ranks; ``trajectories=1`` with an ansatz without channels is ``build_kernel_matrix`` to rounding.  Returns the
    ``len(Y) x len(X)`` matrix on rank 0, ``None`` elsewhere."""
    X, Y, fidelity, T = _noisy_arguments(X, Y, trajectories, noise_seed, truncation_error)
    run = _start(mpi_comm, "the noisy kernels have")
    shares = []  # of the expanded sets: T states per point
    try:
        for label, points, first in (("X", X, 0), ("Y", Y, len(X))):
            if points is None:
                continue
            lo, local, _, noisy = _noisy_share(ansatz, points, first, T, noise_seed, run.rank, run.n_procs, fidelity, run.is_root, label, run.device_id)
            shares.append(_Share(label, len(points) * T, lo * T, local, [], []))
            if Y is None and T < 2 and any(comm_allgather(mpi_comm, bool(noisy))):
                raise ValueError("a symmetric noisy kernel leaves the a = b terms out of its diagonal: it needs trajectories >= 2")
        run.ctx.trim()
        locals_ = [s.local for s in shares]
        with _exchanged(run, mpi_comm, locals_, shares) as full:
            if run.n_procs > 1:  # the full sets are copies: the shares go back before the sweep needs the memory
                _close_all(locals_)
            gram, _ = _gram_of(run, mpi_comm, full)
    finally:
        _close_all(s.local for s in shares)  # (a no-op for sets closed above: ``MpsSet.close`` may be called twice)
    if not run.is_root:
        return None
    ny = len(X) if Y is None else len(Y)
    blocks = np.asarray(gram, dtype=np.float64).reshape(ny, T, len(X), T)  # [j][b][i][a]
    K = blocks.sum(axis=(1, 3)) / float(T * T)
    if Y is None and T >= 2:
        for i in range(len(X)):
            K[i, i] = (blocks[i, :, i, :].sum() - np.trace(blocks[i, :, i, :])) / float(T * (T - 1))
    return K
