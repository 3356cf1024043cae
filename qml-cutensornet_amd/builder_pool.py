"""Build many MPS on the host cores in parallel (input production, outside the hot path).

Stands in for the per-rank ``simulate`` loop of the reference
(/root/reference/gpu_backend/kernel_state_ansatz.py:213-231): every data point
is independent, so the points are dealt to a process pool with BLAS pinned to one
thread per worker.
"""
from __future__ import annotations

import multiprocessing as mp
import os
import time

import numpy as np

from .ansatz import as_bound_circuit, reject_channels
from .mps import MPS, simulate

_G = {}


def _init(ansatz, fidelity, max_bond=None, initial=None):
    for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        os.environ[v] = "1"
    try:
        from threadpoolctl import threadpool_limits

        _G["tp"] = threadpool_limits(1)
    except Exception:  # pragma: no cover - threadpoolctl is optional
        pass
    _G["ansatz"], _G["fid"], _G["chi"], _G["initial"] = ansatz, fidelity, max_bond, initial


def _one(x):
    t0 = time.perf_counter()
    ansatz = _G["ansatz"]
    circuit = as_bound_circuit(ansatz.circuit_for_data(x), ansatz)
    reject_channels([circuit], "build_states")
    m = simulate(circuit, _G["fid"], max_bond=_G.get("chi"))
    return m.tensors, m.fidelity, time.perf_counter() - t0


def _one_from(item):
    """``_one`` for row ``item[0]`` of X, started from its given state."""
    t0 = time.perf_counter()
    k, x = item
    ansatz, initial = _G["ansatz"], _G["initial"]
    circuit = as_bound_circuit(ansatz.circuit_for_data(x), ansatz)
    reject_channels([circuit], "build_states")
    m = simulate(circuit, _G["fid"], max_bond=_G.get("chi"), initial=initial if isinstance(initial, MPS) else initial[k])
    return m.tensors, m.fidelity, time.perf_counter() - t0


def default_workers() -> int:
    """Host cores this process may really use: the affinity mask, clipped by the cgroup CPU
    quota and by QK_BUILD_WORKERS (default cap 16: a GPU box hands each GPU a 16-core share
    even though the affinity mask shows every core of the node)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:  # pragma: no cover
        n = os.cpu_count() or 1
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        if quota != "max":
            n = min(n, max(1, -(-int(quota) // int(period))))
    except (OSError, ValueError):
        pass
    cap = int(os.environ.get("QK_BUILD_WORKERS", "16"))
    return max(1, min(n, cap))


def build_states(ansatz, X, truncation_fidelity, workers=None, max_bond=None, initial=None):
    """Return (list[MPS], per-state build seconds) for the rows of ``X``.  ``initial`` (one ``MPS`` for all rows, or a list with
    one per row) starts the circuits from given states instead of |0...0> (``simulate(..., initial=)``)."""
    X = np.asarray(X, dtype=np.float64)
    workers = default_workers() if workers is None else int(workers)
    workers = min(workers, len(X)) or 1
    if initial is not None and not isinstance(initial, MPS) and len(initial) != len(X):
        raise ValueError(f"build_states: {len(initial)} initial states for {len(X)} data points")
    fn, jobs = (_one, list(X)) if initial is None else (_one_from, list(enumerate(X)))
    if workers <= 1:
        _init(ansatz, truncation_fidelity, max_bond, initial)
        res = [fn(x) for x in jobs]
    else:
        ctx = mp.get_context("fork")
        with ctx.Pool(workers, initializer=_init, initargs=(ansatz, truncation_fidelity, max_bond, initial)) as pool:
            res = pool.map(fn, jobs, chunksize=1)
    return [MPS(t, f) for t, f, _ in res], [dt for _, _, dt in res]
