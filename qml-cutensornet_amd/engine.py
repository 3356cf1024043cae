"""ctypes binding of the C ABI in ``include/qkgram.h`` (library: ``libqkgram.so``, built in-tree
by ``__graft_entry__.build()``).

This is the only door to the hot path.  There is no CPU fallback: if the library
is missing, or no gfx950 device is usable, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from contextlib import contextmanager

import numpy as np

from . import program as _program

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libqkgram.so")

QK_LAYOUT_LPR, QK_LAYOUT_LRP = 0, 1
QK_PLAN_SYMMETRIC = 1
QK_PLAN_QUADS = 2  # 2x2 blocks of pairs per workgroup (include/qkgram.h)
QK_PLAN_ORIENT = 4  # symmetric plans: list each pair in the cheaper order of contraction


class QkError(RuntimeError):
    pass


class QkStats(C.Structure):
    _fields_ = [
        ("pairs", C.c_int64),
        ("flops", C.c_double),
        ("padded_flops", C.c_double),
        ("bytes", C.c_double),
        ("kernel_ms", C.c_double),
        ("grid", C.c_int32),
        ("max_bond", C.c_int32),
        ("kernel", C.c_int32),
        ("precision", C.c_int32),
        ("second_pairs", C.c_int64),
        ("second_flops", C.c_double),
        ("second_padded_flops", C.c_double),
        ("second_bytes", C.c_double),
        ("second_ms", C.c_double),
        ("second_kernel", C.c_int32),
        ("queues", C.c_int32),
        ("tail_frac", C.c_double),
        ("second_tail_frac", C.c_double),
        ("derive_ms", C.c_double),
        ("lds_bytes", C.c_int32),
        ("second_lds_bytes", C.c_int32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_lib = None

# every symbol include/qkgram.h declares: (name, restype, argtypes)
_P = C.c_void_p
# the entries from before qk_build_program, each the one before it plus a group of arguments in front of `out`
_BUILD_ARGS = [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_double, C.c_double, C.c_int32, C.c_uint32]  # ctx .. flags
_SCAN_ARGS = [C.c_int32, _P, _P, C.c_int32]  # n_checkpoints, checkpoints, initial, initial_snapshot
_MATS_ARGS = [C.c_int32, _P, C.c_int32, _P]  # n_mats, mats, mats_state_stride, mat
_CHAN_ARGS = [C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_uint64, _P, _P, C.c_uint32]  # n_channels .. first_gate
_CHAN2_ARGS = [C.c_int32, _P, _P]  # n_channels2, kraus2, n_kraus2
_SIGNATURES = [
    ("qk_last_error", C.c_char_p, []),
    ("qk_device_count", C.c_int, []),
    ("qk_ctx_create", C.c_int, [C.c_int, C.POINTER(_P)]),
    ("qk_ctx_destroy", C.c_int, [_P]),
    ("qk_ctx_set_stream", C.c_int, [_P, _P]),
    ("qk_ctx_use_own_stream", C.c_int, [_P]),
    ("qk_ctx_synchronize", C.c_int, [_P]),
    ("qk_ctx_trim", C.c_int, [_P]),
    ("qk_mps_set_create", C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.POINTER(_P)]),
    ("qk_mps_set_destroy", C.c_int, [_P]),
    ("qk_mps_set_info", C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    ("qk_mps_set_image", C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(_P), _P, _P]),
    ("qk_mps_set_copy_image", C.c_int, [_P, _P, C.c_int64]),
    ("qk_mps_set_from_packed", C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, C.c_int64, C.POINTER(_P)]),
    ("qk_mps_set_precision", C.c_int, [_P]),
    ("qk_mps_set_to_f32", C.c_int, [_P, _P, C.POINTER(_P)]),
    ("qk_mps_set_compress", C.c_int, [_P, _P, C.c_int32, C.c_double, C.c_double, C.POINTER(_P), _P, _P]),
    ("qk_pack_state_size", C.c_int64, [C.c_int32, _P]),
    ("qk_pack_state", C.c_int, [C.c_int32, _P, _P, C.c_int32, _P, _P]),
    ("qk_plan_create", C.c_int, [C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_P)]),
    ("qk_plan_destroy", C.c_int, [_P]),
    ("qk_plan_num_pairs", C.c_int64, [_P]),
    ("qk_plan_total_pairs", C.c_int64, [_P]),
    ("qk_plan_max_pairs_per_rank", C.c_int64, [_P]),
    ("qk_plan_pairs", _P, [_P]),
    ("qk_plan_stats", C.c_int, [_P, C.POINTER(QkStats)]),
    ("qk_plan_first_run", C.c_int64, [_P]),
    ("qk_plan_queues", C.c_int, [_P, _P]),
    ("qk_plan_edge_sites", C.c_int32, [_P]),
    ("qk_plan_create_all", C.c_int, [C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_uint32, C.c_int32, _P]),
    ("qk_plan_cost", C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    ("qk_gram_values", C.c_int, [_P, _P, _P, _P, _P, _P]),
    ("qk_gram_values_host", C.c_int, [_P, _P, _P, _P, _P, _P]),
    ("qk_scatter", C.c_int, [_P, _P, _P, C.c_int64, _P, C.c_int64, C.c_int32]),
    ("qk_gram_host", C.c_int, [_P, _P, _P, _P, C.c_int64]),
    ("qk_overlaps_host", C.c_int, [_P, _P, _P, _P]),
    ("qk_get_stats", C.c_int, [_P, C.POINTER(QkStats)]),
    ("qk_local_paulis_host", C.c_int, [_P, _P, _P, _P]),
    ("qk_projected_gram_host", C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_double, _P, C.c_int64]),
    ("qk_local_pair_paulis_host", C.c_int, [_P, _P, _P, _P, _P]),
    ("qk_projected_pair_gram_host", C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_double, _P, C.c_int64]),
    ("qk_local_pair_paulis_dist_host", C.c_int, [_P, _P, C.c_int32, _P, _P, _P]),
    ("qk_projected_pair_gram_dist_host", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_double, _P, C.c_int64]),
    ("qk_pauli_strings_host", C.c_int, [_P, _P, C.c_int32, _P, _P, _P]),
    ("qk_operator_strings_host", C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P, _P, _P]),
    ("qk_mpo_expectations_host", C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P]),
    ("qk_mps_set_apply_mpo", C.c_int, [_P, _P, _P, _P, C.POINTER(_P)]),
    ("qk_feature_gram_host", C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_double, _P, C.c_int64]),
    ("qk_bond_purities_host", C.c_int, [_P, _P, _P, _P]),
    ("qk_bond_spectra_host", C.c_int, [_P, _P, C.c_int32, _P, _P]),
    ("qk_block_values_host", C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, _P, _P]),
    ("qk_block_self_host", C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    ("qk_window_rdms_host", C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    ("qk_sample_host", C.c_int, [_P, _P, C.c_int32, _P, C.c_uint64, C.c_int64, _P, _P]),
    ("qk_amplitudes_host", C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P, _P, _P, _P, _P]),
    ("qk_shot_block_sums_host", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_int64, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    ("qk_shadow_hist_host", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int64, _P, _P, _P]),
    ("qk_shot_strings_host", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    ("qk_kernel_name", C.c_char_p, [C.c_int32, C.c_int32]),
    ("qk_selftest_mfma", C.c_int, [_P]),
    ("qk_build_mps", C.c_int, _BUILD_ARGS + [C.POINTER(_P)]),
    ("qk_built_info", C.c_int, [_P, _P, _P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    ("qk_built_launch", C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("qk_built_download", C.c_int, [_P, _P]),
    ("qk_built_destroy", C.c_int, [_P]),
    ("qk_mps_set_from_built", C.c_int, [_P, _P, C.POINTER(_P)]),
    ("qk_build_program", C.c_int, [_P, _P, _P, C.POINTER(_P)]),
    ("qk_program_size", C.c_uint32, []),
    ("qk_build_run_size", C.c_uint32, []),
    ("qk_build_mps_scan", C.c_int, _BUILD_ARGS + _SCAN_ARGS + [C.POINTER(_P)]),
    ("qk_build_mps_gates", C.c_int, _BUILD_ARGS + _SCAN_ARGS + _MATS_ARGS + [C.POINTER(_P)]),
    ("qk_build_mps_channels", C.c_int, _BUILD_ARGS + _SCAN_ARGS + _MATS_ARGS + _CHAN_ARGS + [C.POINTER(_P)]),
    ("qk_build_mps_channels2", C.c_int, _BUILD_ARGS + _SCAN_ARGS + _MATS_ARGS + _CHAN_ARGS + _CHAN2_ARGS + [C.POINTER(_P)]),
    ("qk_build_mps_conditions", C.c_int, _BUILD_ARGS + _SCAN_ARGS + _MATS_ARGS + _CHAN_ARGS + _CHAN2_ARGS + [_P, _P, C.POINTER(_P)]),
    ("qk_built_logw_at", C.c_int, [_P, C.c_int32, _P]),
    ("qk_built_num_channel_gates", C.c_int, [_P]),
    ("qk_built_branches", C.c_int, [_P, _P]),
    ("qk_built_num_snapshots", C.c_int, [_P]),
    ("qk_built_checkpoints", C.c_int, [_P, _P]),
    ("qk_built_info_at", C.c_int, [_P, C.c_int32, _P, _P, _P, _P, C.POINTER(C.c_int64)]),
    ("qk_built_download_at", C.c_int, [_P, C.c_int32, _P]),
    ("qk_mps_set_from_built_at", C.c_int, [_P, _P, C.c_int32, C.POINTER(_P)]),
    ("qk_built_from_set", C.c_int, [_P, _P, C.c_int32, _P, C.c_double, C.c_uint32, C.POINTER(_P), _P, _P]),
    ("qk_mps_set_centre", C.c_int, [_P]),
    ("qk_debug_jacobi", C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    ("qk_debug_jacobi_precond", C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    ("qk_range_push", C.c_int, [C.c_char_p]),
    ("qk_range_pop", C.c_int, []),
    ("qk_comm_init_all", C.c_int, [C.c_int32, _P, C.POINTER(_P)]),
    ("qk_comm_destroy", C.c_int, [_P]),
    ("qk_comm_size", C.c_int32, [_P]),
    ("qk_comm_ctx", _P, [_P, C.c_int32]),
    ("qk_mps_set_allgather", C.c_int, [_P, _P, _P, C.c_int32, _P]),
    ("qk_gram_sharded", C.c_int, [_P, _P, _P, _P, C.c_int64]),
    ("qk_comm_device_gram", C.c_int, [_P, C.c_int32, C.POINTER(_P)]),
    ("qk_comm_stats", C.c_int, [_P, C.c_int32, C.POINTER(QkStats), C.POINTER(C.c_double)]),
]
EXPORTED_SYMBOLS = [s[0] for s in _SIGNATURES]
# entry points of lab/qk_lab.h: only the lab library (lab/libqklab.so, loaded by lab/tools via use_lab_library()) has them
_LAB_SIGNATURES = [
    ("qk_debug_profile", C.c_int, [_P, _P]),
    ("qk_debug_mma_bench", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
]
LAB_LIB_PATH = os.path.join(os.path.dirname(_HERE), "lab", "libqklab.so")


def use_lab_library(path=None):
    """lab/tools only: load the lab library (experimental kernels, QK_VARIANT, instrumented builds) instead of the
    shipped one.  Must be called before the first use of the engine."""
    global LIB_PATH
    if _lib is not None:
        raise QkError("use_lab_library() must be called before the library is loaded")
    LIB_PATH = path or os.environ.get("QK_LIB") or LAB_LIB_PATH


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own ``libamdhip64.so``
    (SONAME libamdhip64.so.7, looked up by file name from libtorch_hip.so); libqkgram.so needs
    ``libamdhip64.so.7``.  Loaded in the wrong order the process ends up with two runtimes and
    the second one sees no device.  Loading torch's copy first (if torch is installed) makes
    both resolve to the same object; without torch the system runtime is used."""
    import importlib.util

    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec and spec.origin:
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)


def lib():
    """Load ``libqkgram.so`` (once).  Raises ``QkError`` if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise QkError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the Gram path."
            )
        _preload_hip_runtime()
        L = C.CDLL(LIB_PATH)
        for name, res, args in _SIGNATURES:
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        for name, res, args in _LAB_SIGNATURES:  # present in the lab library only
            if hasattr(L, name):
                f = getattr(L, name)
                f.restype, f.argtypes = res, args
        try:
            _program.check_sizes(L, {"qk_program_size": _program.QkProgram, "qk_build_run_size": _program.QkBuildRun})
        except ImportError as e:
            raise QkError(str(e)) from None
        _lib = L
    return _lib


def _check(rc: int, what: str):
    if rc != 0:
        msg = lib().qk_last_error()
        raise QkError(f"{what}: error {rc}: {msg.decode() if msg else '?'}")


def device_count() -> int:
    return int(lib().qk_device_count())


def range_push(name: str) -> None:
    """Open a roctx range (visible to ``rocprofv3 --marker-trace``; a no-op unless a profiler is attached or QK_ROCTX=1)."""
    lib().qk_range_push(name.encode())


def range_pop() -> None:
    lib().qk_range_pop()


def projected_gamma(gamma, n_sites: int) -> float:
    """The bandwidth g of the projected quantum kernel: ``gamma``, or ``1 / n_sites`` for ``None`` (sum_k ||rho_k - sigma_k||_F^2
    grows like n, and 1/n keeps the exponent O(1)).  Raises ``ValueError`` unless g > 0 and finite."""
    g = 1.0 / int(n_sites) if gamma is None else float(gamma)
    if not (g > 0.0 and np.isfinite(g)):
        raise ValueError(f"the projected-kernel bandwidth must be > 0 and finite (got {gamma!r})")
    return g


def pair_table(n_sites: int, max_dist: int = 1) -> np.ndarray:
    """The qubit pairs of the two-qubit projected kernel, in the order of ``local_pair_paulis(max_dist=...)``: an int array
    (n_pairs, 2) of (k, k + d), d = 1 .. max_dist, k = 0 .. n_sites - 1 - d, distance-major (row ``sum_{e<d} (n_sites - e) + k``);
    n_pairs = D n - D (D + 1) / 2.  For an entanglement map, ``max_dist = max(abs(a - b) for a, b in pairs)``."""
    n, D = int(n_sites), int(max_dist)
    if n < 2 or not 1 <= D <= n - 1:
        raise ValueError(f"max_dist must be in 1 .. n_sites - 1 (got n_sites {n_sites!r}, max_dist {max_dist!r})")
    return np.array([(k, k + d) for d in range(1, D + 1) for k in range(n - d)], dtype=np.int64)


def _pair_sites(n_pairs: int, max_dist: int):
    """n_sites of a feature array with ``n_pairs`` pairs up to distance ``max_dist``, or None if no chain fits."""
    D = int(max_dist)
    if D < 1:
        return None
    n, rem = divmod(int(n_pairs) + D * (D + 1) // 2, D)
    return n if rem == 0 and n >= D + 1 else None


_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
BASIS_CODES = {"X": 1, "Y": 2, "Z": 3}


def philox4x32(counter, key) -> np.ndarray:
    """Philox4x32-10, vectorised: ``counter`` (..., 4) and ``key`` (..., 2) of 32-bit words (broadcast against each other over the
    leading axes) give the four output words, uint32 of shape (..., 4).  Written out here, as in the library's kernels, so that the
    host mirror and the device draw the same bits: ten rounds of
        hi0:lo0 = 0xD2511F53 c0,  hi1:lo1 = 0xCD9E8D57 c2,  (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0)
    with (k0, k1) += (0x9E3779B9, 0xBB67AE85) mod 2^32 before each round after the first."""
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    if c.shape[-1:] != (4,) or k.shape[-1:] != (2,):
        raise ValueError(f"counter must end in 4 words and key in 2 (got shapes {c.shape}, {k.shape})")
    mask = np.uint64(0xFFFFFFFF)
    sh = np.uint64(32)
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., j] & mask, shape) for j in range(4))
    k0, k1 = (np.broadcast_to(k[..., j] & mask, shape) for j in range(2))
    for r in range(10):
        if r > 0:
            k0, k1 = (k0 + np.uint64(_PHILOX_W0)) & mask, (k1 + np.uint64(_PHILOX_W1)) & mask
        p0, p1 = np.uint64(_PHILOX_M0) * c0, np.uint64(_PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & mask, (p0 >> sh) ^ c3 ^ k1, p0 & mask
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _seed_key(seed):
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"seed must be an int in 0 .. 2^64 - 1 (got {seed!r})")
    return np.array([int(seed) & 0xFFFFFFFF, int(seed) >> 32], dtype=np.uint64)


def _philox_stream(seed, state, shot, site, stream):
    state, shot, site = np.broadcast_arrays(np.asarray(state, dtype=np.uint64), np.asarray(shot, dtype=np.uint64), np.asarray(site, dtype=np.uint64))
    counter = np.stack([site, shot, state, np.full(site.shape, stream, dtype=np.uint64)], axis=-1)
    return philox4x32(counter, _seed_key(seed))


def sample_uniform(seed, state, shot, site):
    """The uniform in [0, 1) that decides the outcome of qubit ``site`` in shot ``shot`` of the state with global index ``state``
    (arrays broadcast): Philox counter (site, shot, state, 0), key (seed & 0xffffffff, seed >> 32),
    u = ((x0 >> 5) 2^26 + (x1 >> 6)) 2^-53 from the first two output words."""
    x = _philox_stream(seed, state, shot, site, 0).astype(np.uint64)
    return ((x[..., 0] >> np.uint64(5)) * np.uint64(1 << 26) + (x[..., 1] >> np.uint64(6))).astype(np.float64) * 2.0 ** -53


def channel_uniform(seed, gate, trajectory, state):
    """The uniform in [0, 1) that draws the branch of the Kraus channel at position ``gate`` of the program (counted from the start
    of the uninterrupted circuit: ``first_gate + i``) in trajectory ``trajectory`` of the state with index ``state`` (arrays
    broadcast): Philox counter (gate, trajectory, state, 2), key (seed & 0xffffffff, seed >> 32), u made from the first two output
    words as ``sample_uniform`` makes it.  Stream 2: stream 0 draws shots, stream 1 bases."""
    x = _philox_stream(seed, state, trajectory, gate, 2).astype(np.uint64)
    return ((x[..., 0] >> np.uint64(5)) * np.uint64(1 << 26) + (x[..., 1] >> np.uint64(6))).astype(np.float64) * 2.0 ** -53


def with_noise(gates, channel_name, params, after="all"):
    """A gate list ``(name, qubits, params)`` with the channel ``(channel_name, [q], params)`` behind every gate (``after="all"``) or
    behind every two-qubit gate (``after="two_qubit"``), on each qubit the gate touches, in the order the gate names them.  With
    the name of a two-qubit channel (``Depolarizing2q``, ``CorrelatedPhaseFlip``, ..) and ``after="two_qubit"``, ONE channel
    ``(channel_name, [a, b], params)`` goes behind every two-qubit gate, on its pair as the gate names it: correlated gate noise,
    which no pair of one-qubit channels expresses (``after="all"`` is a ``ValueError`` then).  Gates that are channels themselves
    get none.  A conditional gate ``(name, qubits, params, (g, values))`` passes through with g remapped over the channels put
    in, and the channel behind it takes the gate's condition (noise of a gate that did not run does not act).  The list goes to ``BoundCircuit.from_gates`` / ``as_bound_circuit`` or, with the parameters in the place of the
    angle, to ``CircuitAnsatz``."""
    from .ansatz import _CHANNEL2_NAMES, _CHANNEL_NAMES

    if channel_name not in _CHANNEL_NAMES and channel_name not in _CHANNEL2_NAMES:
        raise ValueError(f"unknown channel {channel_name!r} (supported: {', '.join(_CHANNEL_NAMES + _CHANNEL2_NAMES)})")
    if after not in ("all", "two_qubit"):
        raise ValueError(f"after must be 'all' or 'two_qubit', got {after!r}")
    pair = channel_name in _CHANNEL2_NAMES
    if pair and after == "all":
        raise ValueError(f"the two-qubit channel {channel_name!r} goes behind two-qubit gates only: after must be 'two_qubit'")
    out, moved = [], []  # moved[p]: the position in `out` of gate p of `gates`
    for pos, g in enumerate(gates):
        cond = ()
        if len(g) == 4 and g[3] is not None:
            at, values = g[3]
            if not 0 <= int(at) < pos:
                raise ValueError(f"gate {pos}: condition on gate {at} outside 0..{pos - 1}")
            cond = ((moved[int(at)], values),)
            g = (g[0], g[1], g[2]) + cond
        moved.append(len(out))
        out.append(g)
        name, qubits = g[0], g[1]
        qs = [int(q) for q in (qubits if np.ndim(qubits) else [qubits])]
        if (isinstance(name, str) and (name in _CHANNEL_NAMES or name in _CHANNEL2_NAMES)) or (after == "two_qubit" and len(qs) != 2):
            continue
        if pair:
            out.append((channel_name, qs, params) + cond)
        else:
            out.extend((channel_name, [q], params) + cond for q in qs)
    return out


def random_bases(shots: int, n_qubits: int, seed=0) -> np.ndarray:
    """Random measurement bases of a randomised-measurement protocol: uint8 of shape (shots, n_qubits), codes 1..3 = X, Y, Z,
    ``1 + (x0 % 3)`` of Philox stream 1 with counter (site, shot, 0, 1).  The first rows of a longer table are the shorter table."""
    if int(shots) < 1 or int(n_qubits) < 1:
        raise ValueError(f"shots and n_qubits must be >= 1 (got {shots!r}, {n_qubits!r})")
    x = _philox_stream(seed, 0, np.arange(int(shots))[:, None], np.arange(int(n_qubits))[None, :], 1)
    return (1 + x[..., 0] % np.uint32(3)).astype(np.uint8)


def setting_bases(settings: int, shots_per_setting: int, n_qubits: int, seed=0) -> np.ndarray:
    """The bases table of a randomised-measurement protocol with U = ``settings`` random settings of M = ``shots_per_setting`` shots
    each: ``np.repeat(random_bases(U, n_qubits, seed), M, axis=0)``, uint8 of shape (U M, n_qubits).  Shot ``u M + a`` is shot a of
    setting u; ``Context.sample`` draws its M shots independently (its uniforms differ per shot)."""
    if isinstance(shots_per_setting, bool) or not isinstance(shots_per_setting, (int, np.integer)) or int(shots_per_setting) < 1:
        raise ValueError(f"shots_per_setting must be an int >= 1 (got {shots_per_setting!r})")
    return np.repeat(random_bases(settings, n_qubits, seed), int(shots_per_setting), axis=0)


_POPCOUNT8 = np.array([bin(v).count("1") for v in range(256)], dtype=np.int64)
SHOT_BLOCK_MAX_WIDTH = 32


def _shot_bits(bits, name: str) -> np.ndarray:
    b = np.asarray(bits)
    if b.ndim != 3 or b.dtype.kind not in "iub" or b.shape[2] < 1:
        raise ValueError(f"{name} must be an integer array of shape (n_states, shots, n_qubits), got shape {b.shape}, dtype {b.dtype}")
    return b


def pack_block_words(bits, side="left") -> np.ndarray:
    """The packed word of every shot of ``bits`` (..., n_qubits): uint32 of shape (...), bit k = ``bits[..., k]`` (``side="left"``) or
    ``bits[..., n - 1 - k]`` (``"right"``) for k < min(n, 32), the other bits 0.  Raises ``ValueError`` if one of those entries is
    neither 0 nor 1."""
    b = np.asarray(bits)
    if b.ndim < 1 or b.shape[-1] < 1 or b.dtype.kind not in "iub":
        raise ValueError(f"bits must be an integer array whose last axis is the qubits, got shape {b.shape}, dtype {b.dtype}")
    nb = min(b.shape[-1], SHOT_BLOCK_MAX_WIDTH)
    blk = (b[..., ::-1] if _block_side(side) else b)[..., :nb].astype(np.int64)
    if blk.size and (blk.min() < 0 or blk.max() > 1):
        raise ValueError("bits holds a value other than 0 or 1 among the block's qubits")
    return (blk << np.arange(nb, dtype=np.int64)).sum(axis=-1).astype(np.uint32)


def _shot_widths(widths, n: int) -> np.ndarray:
    w = _block_widths(widths, min(n, SHOT_BLOCK_MAX_WIDTH))
    if w.size < 1 or w[0] < 1 or w[-1] > min(n, SHOT_BLOCK_MAX_WIDTH) or np.any(np.diff(w) <= 0):
        raise ValueError(f"widths must be strictly increasing ints in 1 .. min(n_qubits, 32) = {min(n, SHOT_BLOCK_MAX_WIDTH)}, got {widths!r}")
    return w


def _shot_split(shots: int, settings) -> tuple:
    if isinstance(settings, bool) or not isinstance(settings, (int, np.integer)) or int(settings) < 1 or shots < 1 or shots % int(settings):
        raise ValueError(f"settings must be an int >= 1 that divides the {shots} shots of the tables (got {settings!r})")
    return int(settings), shots // int(settings)


def shot_block_sums(bits_x, bits_y, settings, pairs, widths, side="left", per_setting=False):
    """The integer sums of the randomised-measurement overlap (Elben et al., PRL 124, 010504 (2020)) in plain numpy -- the mirror of
    ``Context.shot_block_sums_host``, the same integers from xor and a popcount table.  ``bits_x`` (nx, U M, n) and ``bits_y``
    (ny, U M, n; ``None``: Y is X) are outcome tables of U = ``settings`` settings of M shots, shot u M + a in setting u; ``pairs``
    (n_pairs, 2) lists (x index, y index).  With s, s' the packed words (``pack_block_words``):
        D_w(s, s')  = popcount((s xor s') & (2^w - 1))
        term_w      = (-1)^D_w 2^(w - D_w)
        S_u[w][p]   = sum_{a,b < M} term_w(X[i][uM+a], Y[j][uM+b])  -  [p is a self pair] M 2^w
        sums[w][p]  = sum_u S_u[w][p]
    A self pair is i == j with ``bits_y=None`` (the a == b terms are removed; it needs M >= 2).  Returns ``sums``, int64 of shape
    (n_widths, n_pairs), and with ``per_setting=True`` also S, int64 (n_widths, n_pairs, U).  ``ValueError`` if U M^2 2^w_max > 2^62."""
    bx = _shot_bits(bits_x, "bits_x")
    by = bx if bits_y is None else _shot_bits(bits_y, "bits_y")
    if by.shape[1:] != bx.shape[1:]:
        raise ValueError(f"bits_x and bits_y differ in shots or qubits: {bx.shape} and {by.shape}")
    U, M = _shot_split(bx.shape[1], settings)
    w = _shot_widths(widths, bx.shape[2])
    if U * M * M > (1 << (62 - int(w[-1]))):
        raise ValueError(f"settings {U} x shots_per_setting {M}^2 x 2^{int(w[-1])} exceeds 2^62: the sums would not fit an int64")
    P = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if P.size and (P.min() < 0 or P[:, 0].max() >= bx.shape[0] or P[:, 1].max() >= by.shape[0]):
        raise ValueError(f"pairs holds an index outside the {bx.shape[0]} x {by.shape[0]} states")
    wx = pack_block_words(bx, side).reshape(bx.shape[0], U, M)
    wy = wx if bits_y is None else pack_block_words(by, side).reshape(by.shape[0], U, M)
    S = np.zeros((w.size, len(P), U), dtype=np.int64)
    for e, (i, j) in enumerate(P):
        self_pair = bits_y is None and i == j
        if self_pair and M < 2:
            raise ValueError(f"pairs[{e}] is the self pair ({i}, {j}): it needs shots_per_setting >= 2")
        d = wx[i][:, :, None] ^ wy[j][:, None, :]  # (U, M, M)
        for wi, wd in enumerate(w):
            m = d & np.uint32(0xFFFFFFFF if wd >= 32 else (1 << int(wd)) - 1)
            D = _POPCOUNT8[m & np.uint32(255)] + _POPCOUNT8[(m >> np.uint32(8)) & np.uint32(255)] + _POPCOUNT8[(m >> np.uint32(16)) & np.uint32(255)] + _POPCOUNT8[m >> np.uint32(24)]
            term = (np.int64(1) << (int(wd) - D)) * (1 - 2 * (D & 1))
            S[wi, e] = term.sum(axis=(1, 2)) - (M << int(wd) if self_pair else 0)
    sums = S.sum(axis=2)
    return (sums, S) if per_setting else sums


def shot_block_estimate(sums, per_setting, settings, shots_per_setting, self_mask):
    """``(O_hat, stderr)`` from the sums of ``shot_block_sums``: with N = M^2 for a cross pair and M (M - 1) for a self pair
    (``self_mask`` over the pairs axis, broadcast),
        O_hat  = sums / (U N)
        stderr = std over the settings of S_u / N (ddof = 1) / sqrt(U)       (nan when U < 2 or ``per_setting`` is None)
    ``sums`` is (..., n_pairs) and ``per_setting`` (..., n_pairs, U).  The spread from setting to setting is what the standard error
    measures: the shots of one setting share their bases."""
    U, M = int(settings), int(shots_per_setting)
    sums = np.asarray(sums)
    N = np.where(np.asarray(self_mask, dtype=bool), M * (M - 1), M * M).astype(np.float64)
    N = np.broadcast_to(N, sums.shape)
    O = sums.astype(np.float64) / (U * N)
    if per_setting is None or U < 2:
        return O, np.full(O.shape, np.nan)
    S = np.asarray(per_setting).astype(np.float64) / N[..., None]
    return O, S.std(axis=-1, ddof=1) / np.sqrt(U)


SHADOW_MAX_QUBITS = 128


def _popcount32(v: np.ndarray) -> np.ndarray:
    """bits set in every element of a uint32 array, as int64 (sums of bit fields: no table, no wider temporary)"""
    v = np.asarray(v, dtype=np.uint32)
    v = v - ((v >> np.uint32(1)) & np.uint32(0x55555555))
    v = (v & np.uint32(0x33333333)) + ((v >> np.uint32(2)) & np.uint32(0x33333333))
    v = (v + (v >> np.uint32(4))) & np.uint32(0x0F0F0F0F)
    return ((v * np.uint32(0x01010101)) >> np.uint32(24)).astype(np.int64)


def pack_shadow_words(bits, bases) -> np.ndarray:
    """The packed record of every shot of ``bits`` (..., n_qubits) measured in ``bases`` (broadcast against ``bits``; codes 1, 2, 3 =
    X, Y, Z): uint32 of shape (..., groups, 3) with groups = ceil(n / 32).  Bit k % 32 of group k // 32 holds the outcome bit
    (plane 0), ``code & 1`` (plane 1) and ``code >> 1`` (plane 2) of qubit k; pad bits are 0 in all planes.  Raises ``ValueError`` on
    a bit other than 0 or 1 or a code outside 1..3."""
    b = np.asarray(bits)
    if b.ndim < 1 or b.shape[-1] < 1 or b.dtype.kind not in "iub":
        raise ValueError(f"bits must be an integer array whose last axis is the qubits, got shape {b.shape}, dtype {b.dtype}")
    c = np.asarray(bases)
    if c.dtype.kind not in "iu":
        raise ValueError(f"bases must be an integer array, got dtype {c.dtype}")
    try:
        c = np.broadcast_to(c, b.shape)
    except ValueError:
        raise ValueError(f"bases of shape {c.shape} do not broadcast against bits of shape {b.shape}") from None
    n = b.shape[-1]
    if n > SHADOW_MAX_QUBITS:
        raise ValueError(f"a shadow record holds at most {SHADOW_MAX_QUBITS} qubits (got {n})")
    b, c = b.astype(np.int64), c.astype(np.int64)
    if b.size and (b.min() < 0 or b.max() > 1):
        raise ValueError("bits holds a value other than 0 or 1")
    if c.size and (c.min() < 1 or c.max() > 3):
        raise ValueError("bases holds a code outside 1..3 = X, Y, Z")
    groups = (n + 31) // 32
    planes = np.zeros(b.shape[:-1] + (groups * 32, 3), dtype=np.int64)
    planes[..., :n, 0], planes[..., :n, 1], planes[..., :n, 2] = b, c & 1, c >> 1
    planes = planes.reshape(b.shape[:-1] + (groups, 32, 3))
    return (planes << np.arange(32, dtype=np.int64)[:, None]).sum(axis=-2).astype(np.uint32)


def _shadow_tables(bits, bases, name: str):
    """(bits (ns, T, n), bases as given, per_state) of one side of a shadow call"""
    b = _shot_bits(bits, "bits_" + name)
    c = np.asarray(bases)
    if c.dtype.kind not in "iu" or c.shape not in (b.shape[1:], b.shape):
        raise ValueError(f"bases_{name} must be an integer array of shape {b.shape[1:]} (shared) or {b.shape} (per state), got shape {c.shape}, dtype {c.dtype}")
    return b, c, int(c.ndim == 3)


def _shadow_d(rx: np.ndarray, ry: np.ndarray) -> np.ndarray:
    """d of records that broadcast against each other, (..., groups, 3) -> (...)"""
    eq = ~(rx[..., 1] ^ ry[..., 1]) & ~(rx[..., 2] ^ ry[..., 2]) & (rx[..., 1] | rx[..., 2])
    return (_popcount32(eq) - 2 * _popcount32(eq & (rx[..., 0] ^ ry[..., 0]))).sum(axis=-1)


def shadow_hist(bits_x, bases_x, bits_y, bases_y, pairs, equal=False):
    """The shot-pair histograms of the classical-shadow kernel (Huang et al., Science 377, eabk3333 (2022)) in plain numpy -- the
    mirror of ``Context.shadow_hist_host``, the same integers from the packed records (``pack_shadow_words``) and a popcount table.
    ``bits_x`` (nx, T_x, n) was measured in ``bases_x``, (T_x, n) shared by every state or (nx, T_x, n) per state; ``bits_y``,
    ``bases_y`` likewise (both ``None``: Y is X); ``pairs`` (n_pairs, 2) lists (x index, y index).  Two shots enter through
        d = #(qubits in the same basis with the same outcome) - #(same basis, other outcome),   sum_k tr(sigma_k sigma'_k) = n/2 + 4.5 d
        H[p, d + n] = #{(t, t') : d(x_i shot t, y_j shot t') = d}          int64 (n_pairs, 2 n + 1), sum_d H[p] = T_x T_y
    ``equal=True`` also returns the histogram over the pairs t = t' alone (it needs T_x == T_y)."""
    bx, cx, _ = _shadow_tables(bits_x, bases_x, "x")
    if bits_y is None:
        if bases_y is not None:
            raise ValueError("bases_y is given but bits_y is None (Y is X)")
        by, cy = bx, cx
    else:
        if bases_y is None:
            raise ValueError("bits_y is given but bases_y is None")
        by, cy, _ = _shadow_tables(bits_y, bases_y, "y")
    n = bx.shape[2]
    if by.shape[2] != n:
        raise ValueError(f"bits_x and bits_y differ in qubits: {bx.shape} and {by.shape}")
    if equal and bx.shape[1] != by.shape[1]:
        raise ValueError(f"equal needs as many shots in x as in y (got {bx.shape[1]} and {by.shape[1]})")
    P = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if P.size and (P.min() < 0 or P[:, 0].max() >= bx.shape[0] or P[:, 1].max() >= by.shape[0]):
        raise ValueError(f"pairs holds an index outside the {bx.shape[0]} x {by.shape[0]} states")
    rx = pack_shadow_words(bx, cx)
    ry = rx if bits_y is None else pack_shadow_words(by, cy)
    H = np.zeros((len(P), 2 * n + 1), dtype=np.int64)
    E = np.zeros_like(H) if equal else None
    for e, (i, j) in enumerate(P):
        rows = max(1, (1 << 21) // max(1, ry.shape[1] * ry.shape[2]))  # x shots at a time: temporaries of a few MiB
        for t0 in range(0, rx.shape[1], rows):
            H[e] += np.bincount((_shadow_d(rx[i][t0 : t0 + rows, None], ry[j][None, :]) + n).ravel(), minlength=2 * n + 1)
        if equal:
            E[e] = np.bincount(_shadow_d(rx[i], ry[j]) + n, minlength=2 * n + 1)
    return (H, E) if equal else H


def shadow_inner(H, n_qubits: int, gamma=1.0, equal=None, weights=None) -> np.ndarray:
    """The weighted mean of a function of d over the shot pairs of a histogram ``H`` (..., 2 n + 1) of ``shadow_hist``:
        inner = sum_d H[..., d + n] w(d) / sum_d H[..., d + n]
    ``weights=None`` is the shadow kernel's inner sum, w(d) = exp(gamma / n (n/2 + 4.5 d)) = exp(gamma / n sum_k tr(sigma_k sigma'_k));
    an array of 2 n + 1 weights (index d + n) or a callable of the integer array d is taken instead.  With ``equal`` (the histogram of
    the pairs t = t') the mean is over ``H - equal``, the T (T - 1) pairs of different shots.  ``H`` alone keeps the Gram of a
    symmetric call positive semi-definite exactly -- it is an inner product of mean feature vectors -- but carries the t = t' pairs,
    which share their bases when the tables were measured in one shared bases table."""
    n = int(n_qubits)
    H = np.asarray(H)
    if H.shape[-1] != 2 * n + 1:
        raise ValueError(f"H must have 2 n + 1 = {2 * n + 1} bins on its last axis, got shape {H.shape}")
    d = np.arange(-n, n + 1)
    if weights is None:
        w = np.exp(float(gamma) / n * (0.5 * n + 4.5 * d))
    elif callable(weights):
        w = np.asarray(weights(d), dtype=np.float64)
    else:
        w = np.asarray(weights, dtype=np.float64)
    if w.shape != (2 * n + 1,):
        raise ValueError(f"weights must give 2 n + 1 = {2 * n + 1} values, got shape {w.shape}")
    if equal is not None:
        H = H - np.asarray(equal)
    return (H * w).sum(axis=-1) / H.sum(axis=-1)


def shadow_kernel(H, n_qubits: int, gamma=1.0, tau=1.0, equal=None) -> np.ndarray:
    """The shadow kernel from shot-pair histograms: ``exp(tau * shadow_inner(H, n_qubits, gamma, equal))`` (the paper: tau = gamma =
    1), pure numpy, any leading shape (..., 2 n + 1)."""
    return np.exp(float(tau) * shadow_inner(H, n_qubits, gamma, equal))


def xeb_fidelity(logp, n_qubits: int, kind: str = "linear") -> np.ndarray:
    """Cross-entropy benchmarking fidelity of measured strings under simulated states, per state: ``logp`` (..., n_strings) is the
    log probability of each string (``Context.amplitudes(..., logp=True)``), the mean runs over the last axis.
        kind="linear":  2^n mean(p) - 1                        (1 for strings drawn from a Porter-Thomas state, 0 for uniform ones)
        kind="log":     n log 2 + gamma_Euler + mean(log p)    (likewise; -inf when a string has probability 0)"""
    n = int(n_qubits)
    lp = np.asarray(logp, dtype=np.float64)
    if lp.ndim < 1 or lp.shape[-1] < 1:
        raise ValueError(f"logp must have at least one string on its last axis, got shape {lp.shape}")
    if n < 1:
        raise ValueError(f"n_qubits must be >= 1 (got {n_qubits!r})")
    if kind == "linear":
        return np.ldexp(np.exp(lp), n).mean(axis=-1) - 1.0
    if kind == "log":
        return n * np.log(2.0) + float(np.euler_gamma) + lp.mean(axis=-1)
    raise ValueError(f"kind must be 'linear' or 'log', got {kind!r}")


def bases_table(bases, shots: int, n_qubits: int) -> np.ndarray:
    """The uint8 table (shots, n_qubits) of basis codes that ``Context.sample`` and ``MPS.sample`` take: ``None`` is all Z, a string
    over ``XYZ`` or a row of ``n_qubits`` codes is shared by every shot, an array (shots, n_qubits) is taken as it is.  Raises
    ``ValueError`` that names ``bases`` for any other shape or letter; the codes themselves are checked where they are used."""
    S, n = int(shots), int(n_qubits)
    if bases is None:
        return np.full((S, n), 3, dtype=np.uint8)
    if isinstance(bases, str):
        if len(bases) != n or any(ch not in BASIS_CODES for ch in bases.upper()):
            raise ValueError(f"bases {bases!r} is not a string of {n} letters over XYZ")
        bases = [BASIS_CODES[ch] for ch in bases.upper()]
    b = np.asarray(bases)
    if b.dtype.kind not in "iu" or b.shape not in ((n,), (S, n)):
        raise ValueError(f"bases must be None, a string or integer row of length {n}, or an integer array of shape ({S}, {n}); got shape {b.shape}, dtype {b.dtype}")
    if b.size and (b.min() < 0 or b.max() > 255):
        raise ValueError(f"bases holds a code outside 1..3 = X, Y, Z ({int(b.min() if b.min() < 0 else b.max())})")
    return np.ascontiguousarray(np.broadcast_to(b.astype(np.uint8), (S, n)))


def _bits_and_bases(bits, bases):
    bits = np.asarray(bits)
    if bits.ndim != 3:
        raise ValueError(f"bits must have shape (n_states, shots, n_qubits), got {bits.shape}")
    B = bases_table(bases, bits.shape[1], bits.shape[2])
    if B.size and (B.min() < 1 or B.max() > 3):
        raise ValueError("bases holds a code outside 1..3 = X, Y, Z")
    return 1 - 2 * bits.astype(np.int64), B


def estimate_paulis(bits, bases):
    """Bloch vectors estimated from measurement shots: ``(F_hat, counts)``.  ``bits`` is (n_states, shots, n_qubits) of
    ``Context.sample`` and ``bases`` what it was drawn in.  ``F_hat[s, k, c]`` (n_states, n_qubits, 3) is the mean of ``1 - 2 bit``
    over the shots with ``bases[shot, k] == c + 1``, and 0.0 where no shot has that basis; ``counts[k, c]`` (n_qubits, 3) is the
    number of those shots.  The sums are integers, so the estimate does not depend on the order of the shots."""
    sign, B = _bits_and_bases(bits, bases)
    ns, _, n = sign.shape
    F = np.zeros((ns, n, 3), dtype=np.float64)
    counts = np.zeros((n, 3), dtype=np.int64)
    for c in range(3):
        mask = B == c + 1
        counts[:, c] = mask.sum(axis=0)
        tot = (sign * mask[None]).sum(axis=1)
        F[:, :, c] = np.where(counts[:, c] > 0, tot / np.maximum(counts[:, c], 1), 0.0)
    return F, counts


def estimate_pair_paulis(bits, bases, max_dist: int = 1) -> np.ndarray:
    """Pauli correlators estimated from measurement shots, in ``pair_table(n_qubits, max_dist)`` order: ``T_hat`` of shape
    (n_states, n_pairs, 4, 4).  ``T[0][0] = 1.0`` exactly; ``T[p][0]`` and ``T[0][q]`` are the entries of ``estimate_paulis``;
    ``T[p][q]`` is the mean of the product of the two signs over the shots whose bases on the two qubits are (p, q), and 0.0
    where there is none."""
    sign, B = _bits_and_bases(bits, bases)
    ns, _, n = sign.shape
    F, _ = estimate_paulis(bits, B)
    pairs = pair_table(n, max_dist)
    T = np.zeros((ns, len(pairs), 4, 4), dtype=np.float64)
    for pi, (a, b) in enumerate(pairs):
        T[:, pi, 0, 0] = 1.0
        T[:, pi, 1:, 0] = F[:, a]
        T[:, pi, 0, 1:] = F[:, b]
        prod = sign[:, :, a] * sign[:, :, b]
        for p in range(1, 4):
            for q in range(1, 4):
                mask = (B[:, a] == p) & (B[:, b] == q)
                cnt = int(mask.sum())
                if cnt:
                    T[:, pi, p, q] = (prod * mask[None]).sum(axis=1) / cnt
    return T


def pauli_strings(n_sites: int, specs) -> np.ndarray:
    """Pauli strings as the uint8 code table (m, n_sites) of ``Context.pauli_expectations`` (0..3 = I, X, Y, Z on qubit k).  A spec
    is a ``str`` of length ``n_sites`` over ``IXYZ`` (``"IZXXZI"``), a pair ``(paulis, qubits)`` with distinct qubits in range
    (``("ZXZ", (3, 4, 5))``, identity elsewhere), or an integer row of ``n_sites`` codes; an integer array (m, n_sites) is a
    list of rows.  Raises ``ValueError`` that names the offending spec otherwise."""
    n = int(n_sites)
    if n < 1:
        raise ValueError(f"n_sites must be >= 1 (got {n_sites!r})")
    if isinstance(specs, str) or (isinstance(specs, tuple) and len(specs) == 2 and isinstance(specs[0], str) and not isinstance(specs[1], str)):
        raise ValueError(f"pauli_strings takes a list of specs, got the single spec {specs!r}")
    letters = {"I": 0, "X": 1, "Y": 2, "Z": 3}
    rows = []
    for spec in specs:
        bad = ValueError(f"bad Pauli string {spec!r}: want a str of length {n} over IXYZ, a pair (paulis, qubits) with distinct qubits "
                         f"in 0 .. {n - 1}, or {n} integer codes 0..3")
        row = np.zeros(n, dtype=np.uint8)
        if isinstance(spec, str):
            if len(spec) != n or any(ch not in letters for ch in spec):
                raise bad
            row[:] = [letters[ch] for ch in spec]
        elif isinstance(spec, tuple) and len(spec) == 2 and isinstance(spec[0], str):
            paulis, qubits = spec
            try:
                qubits = [int(q) for q in qubits]
            except (TypeError, ValueError):
                raise bad from None
            if len(qubits) != len(paulis) or len(set(qubits)) != len(qubits) or any(ch not in letters for ch in paulis) or any(not 0 <= q < n for q in qubits):
                raise bad
            for ch, q in zip(paulis, qubits):
                row[q] = letters[ch]
        else:
            try:
                codes = np.asarray(spec)
            except (TypeError, ValueError):
                raise bad from None
            if codes.dtype.kind not in "iu" or codes.shape != (n,) or codes.min() < 0 or codes.max() > 3:
                raise bad
            row[:] = codes
        rows.append(row)
    if not rows:
        raise ValueError("the list of Pauli strings is empty")
    return np.ascontiguousarray(np.stack(rows))


def _local_ops() -> dict:
    h = 0.5
    return {
        "I": [[1, 0], [0, 1]], "X": [[0, 1], [1, 0]], "Y": [[0, -1j], [1j, 0]], "Z": [[1, 0], [0, -1]],
        "0": [[1, 0], [0, 0]], "1": [[0, 0], [0, 1]],            # (I +- Z) / 2
        "+": [[h, h], [h, h]], "-": [[h, -h], [-h, h]],          # (I +- X) / 2
        "R": [[h, -h * 1j], [h * 1j, h]], "L": [[h, h * 1j], [-h * 1j, h]],  # (I +- Y) / 2
        "01": [[0, 1], [0, 0]], "10": [[0, 0], [1, 0]],          # |0><1|, |1><0|
    }


# Named single-site operators, O[s'][s] = <s'|O|s>: the Paulis, the six projectors onto the +1 / -1 eigenstates of Z ("0", "1"), X
# ("+", "-") and Y ("R", "L") -- eigenvalue +1 is outcome bit 0, as in the sampler -- and the two ladder operators.
LOCAL_OPS = {name: np.array(m, dtype=np.complex128) for name, m in _local_ops().items()}
OPERATOR_TABLE_MAX = 255  # operators of one table (qk_operator_strings_host): a code is a byte
_PROJECTOR_NAMES = (("+", "-"), ("R", "L"), ("0", "1"))  # basis code 1..3 = X, Y, Z -> the names of outcome bit 0, 1


def _operator_table(table) -> np.ndarray:
    try:
        t = np.asarray(table, dtype=np.complex128)
    except (TypeError, ValueError):
        raise ValueError("the operator table is not an array of 2 x 2 complex matrices") from None
    if t.ndim != 3 or t.shape[1:] != (2, 2) or not 1 <= t.shape[0] <= OPERATOR_TABLE_MAX:
        raise ValueError(f"the operator table must have shape (n_ops, 2, 2) with 1 <= n_ops <= {OPERATOR_TABLE_MAX}, got {t.shape}")
    if not np.isfinite(t).all():
        c, sp, s0 = (int(v) for v in np.argwhere(~np.isfinite(t.real) | ~np.isfinite(t.imag))[0])
        raise ValueError(f"operator {c + 1} of the table has an entry [{sp}][{s0}] that is not finite")
    return np.ascontiguousarray(t)


def operator_strings(n_sites: int, specs, ops=None):
    """Strings of single-site operators as ``(table, codes)`` for ``Context.operator_expectations`` and
    ``MPS.operator_expectation``: ``table`` complex128 (n_ops, 2, 2) with ``table[c - 1][s'][s] = <s'|O_c|s>`` and ``codes`` uint8
    (m, n_sites), code 0 = the identity, code c = ``table[c - 1]`` on qubit k.  A spec is a pair ``(names, qubits)`` with distinct
    qubits in range, identity elsewhere: ``names`` is a ``str`` of one-letter names (``("0+R", (1, 4, 5))``) or a sequence of
    names (``(("01", "10"), (2, 7))``), taken from ``ops`` first -- a dict ``{name: 2 x 2 array}`` -- and then from ``LOCAL_OPS``;
    the table holds the operators that are used, in the order of first use, and ``"I"`` is code 0.  With ``ops`` an array
    (n_ops, 2, 2), a spec is an integer row of ``n_sites`` codes 0 .. n_ops into that table (an integer array (m, n_sites) is a
    list of rows) and the table is returned as it is.  Raises ``ValueError`` that names the offending spec otherwise."""
    n = int(n_sites)
    if n < 1:
        raise ValueError(f"n_sites must be >= 1 (got {n_sites!r})")
    if isinstance(specs, str) or (isinstance(specs, tuple) and len(specs) == 2 and isinstance(specs[0], str) and not isinstance(specs[1], str)):
        raise ValueError(f"operator_strings takes a list of specs, got the single spec {specs!r}")
    user_table = None
    named = {}
    if isinstance(ops, dict):
        for name, mat in ops.items():
            try:
                m = np.asarray(mat, dtype=np.complex128)
            except (TypeError, ValueError):
                m = None
            if not isinstance(name, str) or not name or m is None or m.shape != (2, 2) or not np.isfinite(m).all():
                raise ValueError(f"ops[{name!r}] is not a finite 2 x 2 matrix under a non-empty str name")
            named[name] = m
    elif ops is not None:
        user_table = _operator_table(ops)
    table, code_of, rows = [], {}, []

    def code(name, bad):
        if name not in named and name not in LOCAL_OPS:
            raise bad
        if name not in named and name == "I":
            return 0
        if name not in code_of:
            if len(table) == OPERATOR_TABLE_MAX:
                raise ValueError(f"the specs use more than {OPERATOR_TABLE_MAX} distinct operators (at {name!r})")
            table.append(named[name] if name in named else LOCAL_OPS[name])
            code_of[name] = len(table)
        return code_of[name]

    for spec in specs:
        top = len(user_table) if user_table is not None else 0
        bad = ValueError(f"bad operator string {spec!r}: want a pair (names, qubits) with distinct qubits in 0 .. {n - 1} and names from ops or LOCAL_OPS"
                         + (f", or {n} integer codes 0..{top} into the table" if user_table is not None else ""))
        row = np.zeros(n, dtype=np.uint8)
        if isinstance(spec, tuple) and len(spec) == 2 and (isinstance(spec[0], str) or (isinstance(spec[0], (tuple, list)) and all(isinstance(v, str) for v in spec[0]))):
            if user_table is not None:
                raise bad
            names, qubits = spec
            try:
                qubits = [int(q) for q in qubits]
            except (TypeError, ValueError):
                raise bad from None
            if len(qubits) != len(names) or len(set(qubits)) != len(qubits) or any(not 0 <= q < n for q in qubits):
                raise bad
            for name, q in zip(names, qubits):
                row[q] = code(name, bad)
        else:
            try:
                codes = np.asarray(spec)
            except (TypeError, ValueError):
                raise bad from None
            if user_table is None or codes.dtype.kind not in "iu" or codes.shape != (n,) or codes.min() < 0 or codes.max() > top:
                raise bad
            row[:] = codes
        rows.append(row)
    if not rows:
        raise ValueError("the list of operator strings is empty")
    if user_table is None:
        user_table = np.stack(table) if table else LOCAL_OPS["I"][None].copy()  # only identities: a table must not be empty
    return np.ascontiguousarray(user_table), np.ascontiguousarray(np.stack(rows))


def marginal_strings(bits, bases, n_sites: int):
    """The projector strings of outcome marginals, as ``(table, codes)`` of ``operator_strings``: ``bits`` (n_strings, n_sites) of
    0 / 1, ``bases`` (n_strings, n_sites) or one shared row of codes 0..3 -- 0: not measured (traced out; the bit there is
    ignored), 1, 2, 3: measured in X, Y, Z.  The table is the six projectors in the order ``+ - R L 0 1``: code ``2 (basis - 1) +
    bit + 1``.  Raises ``ValueError`` that names ``bits`` or ``bases`` otherwise."""
    n = int(n_sites)
    b = np.asarray(bits)
    if b.dtype.kind not in "iub" or b.ndim != 2 or b.shape[1] != n or b.shape[0] < 1:
        raise ValueError(f"bits must be an integer array of shape (n_strings >= 1, {n}); got shape {b.shape}, dtype {b.dtype}")
    B = np.asarray(bases)
    if B.dtype.kind not in "iu" or B.shape not in ((n,), b.shape):
        raise ValueError(f"bases must be an integer row of length {n} or an integer array of shape {b.shape}; got shape {B.shape}, dtype {B.dtype}")
    if B.min() < 0 or B.max() > 3:
        raise ValueError(f"bases holds a code outside 0..3 = not measured, X, Y, Z ({int(B.min() if B.min() < 0 else B.max())})")
    B = np.broadcast_to(B, b.shape)
    if ((b < 0) | (b > 1))[B > 0].any():
        raise ValueError("bits holds a value that is not 0 or 1 on a measured qubit")
    table = np.stack([LOCAL_OPS[name] for pair in _PROJECTOR_NAMES for name in pair])
    codes = np.where(B > 0, 2 * (B.astype(np.int64) - 1) + (b.astype(np.int64) & 1) + 1, 0).astype(np.uint8)
    return table, np.ascontiguousarray(codes)


MPO_MAX_BOND = 32  # the largest bond of an MPO (qk_mpo_expectations_host)
_MPO_DENSE_MAX = 12  # sites of Mpo.to_dense


class Mpo:
    """A matrix-product operator on ``n_sites`` qubits: ``tensors[k]`` is complex128 of shape (w_k, w_{k+1}, 2, 2),
    ``W_k[u][v][s'][s] = <s'| . |s>`` (physical index 0 = |0>, site k = qubit k), with w_0 = w_n = 1 and every bond in
    1 .. ``MPO_MAX_BOND``.  The operator is ``H = sum_{u_1 .. u_{n-1}} (x)_k W_k[u_k][u_{k+1}]``; it need not be Hermitian.
    ``bonds`` is the int32 row (w_0, .., w_n).  ``+`` is the direct sum of the bonds, ``@`` the operator product (bonds multiply),
    ``scale(c)`` puts a factor on the first site, ``dagger()`` is the adjoint, ``to_dense()`` the 2^n x 2^n matrix (qubit 0 the
    most significant bit) for n <= 12.  Evaluate with ``Context.mpo_expectations`` or ``MPS.mpo_expectation``."""

    def __init__(self, tensors):
        try:
            ts = [np.ascontiguousarray(t, dtype=np.complex128) for t in tensors]
        except (TypeError, ValueError):
            raise ValueError("an Mpo takes a sequence of complex arrays of shape (w_k, w_k+1, 2, 2)") from None
        if not ts:
            raise ValueError("an Mpo needs at least one site")
        for k, t in enumerate(ts):
            if t.ndim != 4 or t.shape[2:] != (2, 2) or t.shape[0] < 1 or t.shape[1] < 1:
                raise ValueError(f"Mpo tensor {k} must have shape (w_k, w_k+1, 2, 2), got {t.shape}")
            if k and t.shape[0] != ts[k - 1].shape[1]:
                raise ValueError(f"Mpo tensor {k} has left bond {t.shape[0]}, tensor {k - 1} has right bond {ts[k - 1].shape[1]} (cut {k})")
            if not np.isfinite(t).all():
                u, v, sp, s0 = (int(x) for x in np.argwhere(~np.isfinite(t.real) | ~np.isfinite(t.imag))[0])
                raise ValueError(f"Mpo tensor {k} has an entry [{u}][{v}][{sp}][{s0}] that is not finite")
        if ts[0].shape[0] != 1 or ts[-1].shape[1] != 1:
            raise ValueError(f"an Mpo starts and ends with bond 1, got {ts[0].shape[0]} and {ts[-1].shape[1]}")
        bonds = [1] + [t.shape[1] for t in ts]
        for k, w in enumerate(bonds):
            if w > MPO_MAX_BOND:
                raise ValueError(f"the Mpo has bond {w} at cut {k}, above MPO_MAX_BOND = {MPO_MAX_BOND}")
        self.tensors = ts
        self.bonds = np.array(bonds, dtype=np.int32)
        self.n_sites = len(ts)

    def __len__(self):
        return self.n_sites

    def max_bond(self) -> int:
        return int(self.bonds.max())

    def packed(self) -> np.ndarray:
        """The tensors as qk_mpo_expectations_host takes them: site-major [w_k][w_k+1][2][2][re, im], float64."""
        return np.concatenate([t.reshape(-1) for t in self.tensors]).view(np.float64)

    def to_dense(self) -> np.ndarray:
        n = self.n_sites
        if n > _MPO_DENSE_MAX:
            raise ValueError(f"to_dense is for at most {_MPO_DENSE_MAX} sites, the Mpo has {n}")
        M = np.ones((1, 1, 1), dtype=np.complex128)  # [row][column][bond]
        for t in self.tensors:
            M = np.einsum("rcu,uvps->rpcsv", M, t).reshape(M.shape[0] * 2, M.shape[1] * 2, t.shape[1])
        return np.ascontiguousarray(M[:, :, 0])

    def scale(self, c) -> "Mpo":
        c = complex(c)
        if not np.isfinite(c):
            raise ValueError(f"scale takes a finite factor, got {c!r}")
        return Mpo([self.tensors[0] * c] + self.tensors[1:])

    def dagger(self) -> "Mpo":
        return Mpo([t.conj().transpose(0, 1, 3, 2) for t in self.tensors])

    def _same_sites(self, other, what):
        if not isinstance(other, Mpo):
            raise TypeError(f"{what} takes two Mpo, got {type(other).__name__}")
        if other.n_sites != self.n_sites:
            raise ValueError(f"{what}: the two Mpo have {self.n_sites} and {other.n_sites} sites")

    def __add__(self, other) -> "Mpo":
        self._same_sites(other, "+")
        n, out = self.n_sites, []
        for k, (a, b) in enumerate(zip(self.tensors, other.tensors)):
            if n == 1:
                out.append(a + b)
                continue
            la, ra = (0 if k == 0 else a.shape[0]), (0 if k == n - 1 else a.shape[1])
            t = np.zeros(((1 if k == 0 else a.shape[0] + b.shape[0]), (1 if k == n - 1 else a.shape[1] + b.shape[1]), 2, 2), dtype=np.complex128)
            t[: a.shape[0], : a.shape[1]] = a
            t[la:, ra:] = b
            out.append(t)
        return Mpo(out)

    def __matmul__(self, other) -> "Mpo":
        self._same_sites(other, "@")
        return Mpo([np.einsum("uvpq,xyqs->uxvyps", a, b).reshape(a.shape[0] * b.shape[0], a.shape[1] * b.shape[1], 2, 2) for a, b in zip(self.tensors, other.tensors)])


def _mpo_list(mpos, n_sites: int):
    if isinstance(mpos, Mpo):
        raise ValueError("expected a list of Mpo, got a single Mpo")
    ms = list(mpos)
    if not ms:
        raise ValueError("the list of MPOs is empty")
    for j, m in enumerate(ms):
        if not isinstance(m, Mpo):
            raise ValueError(f"entry {j} of the list is not an Mpo ({type(m).__name__})")
        if m.n_sites != n_sites:
            raise ValueError(f"Mpo {j} has {m.n_sites} sites, the states have {n_sites}")
    return ms


def mpo_product(n_sites: int, names_or_table, qubits=None) -> Mpo:
    """The bond-1 MPO of one operator string, in the specs of ``operator_strings``: ``mpo_product(n, names, qubits)`` with names
    from ``LOCAL_OPS`` (a ``str`` of one-letter names or a sequence of names), or ``mpo_product(n, table, codes)`` with a table
    (n_ops, 2, 2) and a row of ``n`` integer codes (0 = identity).  A site without an operator holds the exact 1 x 1 identity."""
    if isinstance(names_or_table, str) or (isinstance(names_or_table, (tuple, list)) and all(isinstance(v, str) for v in names_or_table)):
        table, codes = operator_strings(n_sites, [(names_or_table if isinstance(names_or_table, str) else tuple(names_or_table), tuple(qubits))])
    else:
        table, codes = operator_strings(n_sites, [np.asarray(qubits)], ops=names_or_table)
    eye = np.eye(2, dtype=np.complex128)
    return Mpo([(table[c - 1] if c else eye).reshape(1, 1, 2, 2) for c in codes[0]])


def mpo_from_terms(n_sites: int, terms, ops=None) -> Mpo:
    """The exact finite-state machine of ``sum_t coeff_t O_t``: ``terms = [(coeff, names, qubits), ...]`` with ``(names, qubits)`` a
    spec of ``operator_strings`` (names from ``ops``, a dict, and ``LOCAL_OPS``).  The states at the cut in front of site k are, in
    this order: ``start`` if a term begins at a site >= k, one state per term with first < k <= last in term order, then ``done``
    if a term ends before k.  ``W[start][start] = W[done][done] = I``; the coefficient sits on the term's first site; identity
    sits on the sites of a term's hull that it does not act on; one-site terms add into ``W[start][done]``.  Duplicate terms are
    allowed.  A cut with more than ``MPO_MAX_BOND`` states is a ``ValueError`` that names the cut."""
    n = int(n_sites)
    terms = list(terms)
    if not terms:
        raise ValueError("the list of terms is empty")
    specs, coeffs = [], []
    for j, term in enumerate(terms):
        if not isinstance(term, (tuple, list)) or len(term) != 3:
            raise ValueError(f"term {j} is not a triple (coeff, names, qubits): {term!r}")
        try:
            c = complex(term[0])
        except (TypeError, ValueError):
            raise ValueError(f"term {j} has a coefficient that is not a number: {term[0]!r}") from None
        if not np.isfinite(c):
            raise ValueError(f"term {j} has a coefficient that is not finite: {term[0]!r}")
        coeffs.append(c)
        specs.append((term[1] if isinstance(term[1], str) else tuple(term[1]), tuple(term[2])))
    table, codes = operator_strings(n, specs, ops)
    eye = np.eye(2, dtype=np.complex128)
    first, last = [], []
    for j, row in enumerate(codes):
        nz = np.flatnonzero(row)
        if nz.size == 0:
            raise ValueError(f"term {j} acts on no qubit: {terms[j]!r}")
        first.append(int(nz[0])), last.append(int(nz[-1]))

    def states(k):  # of the cut in front of site k
        s = ["start"] if any(f >= k for f in first) else []
        s += [j for j in range(len(terms)) if first[j] < k <= last[j]]
        return s + (["done"] if any(e < k for e in last) else [])

    cuts = [states(k) for k in range(n + 1)]
    for k, s in enumerate(cuts):
        if len(s) > MPO_MAX_BOND:
            raise ValueError(f"the terms need {len(s)} states at cut {k}, above MPO_MAX_BOND = {MPO_MAX_BOND}")
    tensors = []
    for k in range(n):
        li, ri = {s: i for i, s in enumerate(cuts[k])}, {s: i for i, s in enumerate(cuts[k + 1])}
        W = np.zeros((len(li), len(ri), 2, 2), dtype=np.complex128)
        if "start" in li and "start" in ri:
            W[li["start"], ri["start"]] = eye
        if "done" in li and "done" in ri:
            W[li["done"], ri["done"]] = eye
        for j, row in enumerate(codes):
            if not first[j] <= k <= last[j]:
                continue
            o = table[row[k] - 1] if row[k] else eye
            src = li["start"] if k == first[j] else li[j]
            dst = ri["done"] if k == last[j] else ri[j]
            W[src, dst] += coeffs[j] * o if k == first[j] else o
        tensors.append(W)
    return Mpo(tensors)


def mpo_exponential(n_sites: int, a, b, J, lam) -> Mpo:
    """``sum_{i<j} J lam^(j-i-1) a_i b_j`` as an MPO of bond 3 (states start, open, done): ``a`` and ``b`` are names of
    ``LOCAL_OPS`` or 2 x 2 matrices.  ``n_sites >= 2``."""
    n = int(n_sites)
    if n < 2:
        raise ValueError(f"mpo_exponential needs n_sites >= 2 (got {n_sites!r})")

    def op(x, what):
        if isinstance(x, str):
            if x not in LOCAL_OPS:
                raise ValueError(f"{what} = {x!r} is not a name of LOCAL_OPS")
            return LOCAL_OPS[x]
        m = np.asarray(x, dtype=np.complex128)
        if m.shape != (2, 2) or not np.isfinite(m).all():
            raise ValueError(f"{what} is not a finite 2 x 2 matrix")
        return m

    A, B, J, lam = op(a, "a"), op(b, "b"), complex(J), complex(lam)
    if not (np.isfinite(J) and np.isfinite(lam)):
        raise ValueError("J and lam must be finite")
    eye = np.eye(2, dtype=np.complex128)
    W = np.zeros((3, 3, 2, 2), dtype=np.complex128)
    W[0, 0], W[0, 1], W[1, 1], W[1, 2], W[2, 2] = eye, J * A, lam * eye, B, eye

    def states(k):  # of the cut in front of site k: start while a pair can still begin, open between the two ends, done behind an end
        return [i for i, there in ((0, k <= n - 2), (1, 1 <= k <= n - 1), (2, k >= 2)) if there]

    return Mpo([W[np.ix_(states(k), states(k + 1))] for k in range(n)])


def _mpo_qubits(n: int, qubits, what: str) -> list:
    try:
        qs = [int(q) for q in qubits]
    except (TypeError, ValueError):
        raise ValueError(f"{what}: qubits must be a sequence of ints, got {qubits!r}") from None
    if not qs:
        raise ValueError(f"{what}: the list of qubits is empty")
    if len(set(qs)) != len(qs):
        raise ValueError(f"{what}: a qubit is named twice in {qs}")
    for q in qs:
        if not 0 <= q < n:
            raise ValueError(f"{what}: qubit {q} is outside a register of {n}")
    return qs


def mpo_parity_projector(n_sites: int, sign=+1, qubits=None) -> Mpo:
    """The projector ``(1 + sign prod_{q in qubits} Z_q) / 2`` on the even (sign = +1) or odd (sign = -1) parity sector of
    ``qubits`` (default: all).  Bond 2 inside the hull of ``qubits`` (state 0 carries the identity, state 1 the Z string; both
    factors 1/2 sit on the first site of the hull), the exact 1 x 1 identity outside; a single qubit gives bond 1."""
    n = int(n_sites)
    if n < 1:
        raise ValueError(f"mpo_parity_projector needs n_sites >= 1 (got {n_sites!r})")
    if isinstance(sign, bool) or sign not in (1, -1):
        raise ValueError(f"sign must be +1 or -1, got {sign!r}")
    qs = set(_mpo_qubits(n, range(n) if qubits is None else qubits, "mpo_parity_projector"))
    lo, hi = min(qs), max(qs)
    eye, Z = np.eye(2, dtype=np.complex128), LOCAL_OPS["Z"]
    tensors = []
    for k in range(n):
        z = Z if k in qs else eye
        if k < lo or k > hi:
            W = eye.reshape(1, 1, 2, 2)
        elif lo == hi:
            W = (0.5 * (eye + sign * Z)).reshape(1, 1, 2, 2)
        elif k == lo:
            W = np.stack([0.5 * eye, 0.5 * sign * z]).reshape(1, 2, 2, 2)
        elif k == hi:
            W = np.stack([eye, z]).reshape(2, 1, 2, 2)
        else:
            W = np.zeros((2, 2, 2, 2), dtype=np.complex128)
            W[0, 0], W[1, 1] = eye, z
        tensors.append(W)
    return Mpo(tensors)


def mpo_two_qubit_gate(n_sites: int, a: int, b: int, U) -> Mpo:
    """A 4 x 4 matrix on qubits (a, b), any distance apart, as an MPO in operator-Schmidt form: ``U = sum_j sigma_j L_j (x) R_j``
    with ``U`` in the index convention of ``Unitary2q`` (index (s_a, s_b), a most significant; rows are the outcome).  Terms with
    ``sigma_j <= 1e-14 sigma_0`` are dropped, so the bond is the operator-Schmidt rank (<= 4; 2 for CX); ``sigma_j L_j`` sits on
    the lower qubit, ``R_j`` on the higher one, the identity carries each kept term over the sites between them, and the sites
    outside hold the exact 1 x 1 identity.  For a > b the two qubit roles are exchanged, as ``Unitary2q`` does.  ``U`` need not be
    unitary."""
    n = int(n_sites)
    a, b = _mpo_qubits(n, (a, b), "mpo_two_qubit_gate")
    try:
        M = np.asarray(U, dtype=np.complex128)
    except (TypeError, ValueError):
        raise ValueError("mpo_two_qubit_gate: U is not a 4 x 4 matrix") from None
    if M.shape != (4, 4) or not np.isfinite(M).all():
        raise ValueError(f"mpo_two_qubit_gate: U must be a finite 4 x 4 matrix, got shape {M.shape}")
    T = M.reshape(2, 2, 2, 2)  # [p_a][p_b][s_a][s_b]
    if a > b:
        T, a, b = T.transpose(1, 0, 3, 2), b, a
    u, sig, vh = np.linalg.svd(T.transpose(0, 2, 1, 3).reshape(4, 4))  # [(p_lo, s_lo)][(p_hi, s_hi)]
    if not sig[0] > 0.0:
        raise ValueError("mpo_two_qubit_gate: U is zero")
    r = int((sig > 1e-14 * sig[0]).sum())
    eye = np.eye(2, dtype=np.complex128)
    tensors = []
    for k in range(n):
        if k < a or k > b:
            W = eye.reshape(1, 1, 2, 2)
        elif k == a:
            W = (u[:, :r] * sig[:r]).T.reshape(1, r, 2, 2)
        elif k == b:
            W = vh[:r].reshape(r, 1, 2, 2)
        else:
            W = np.zeros((r, r, 2, 2), dtype=np.complex128)
            W[np.arange(r), np.arange(r)] = eye
        tensors.append(np.ascontiguousarray(W))
    return Mpo(tensors)


def _spectra_array(spectra) -> np.ndarray:
    w = np.asarray(spectra, dtype=np.float64)
    if w.ndim < 1:
        raise ValueError(f"spectra must be an array (..., max_values) of Schmidt weights, got shape {w.shape}")
    return w


def bond_entropies(spectra, alpha: float = 1.0) -> np.ndarray:
    """Entanglement entropies of Schmidt weights (``Context.bond_spectra``) along the last axis, natural logarithm: the von
    Neumann entropy S_1 = -sum lambda log lambda at ``alpha=1``, otherwise the Renyi entropy S_alpha = log(sum lambda^alpha) /
    (1 - alpha) (S_2 = -log purity).  ``alpha`` must be > 0; zero weights (the fill beyond a bond) contribute 0."""
    a = float(alpha)
    if not (a > 0.0 and np.isfinite(a)):
        raise ValueError(f"alpha must be > 0 and finite (got {alpha!r})")
    w = _spectra_array(spectra)
    pos = w > 0.0
    safe = np.where(pos, w, 1.0)
    if a == 1.0:
        return -(np.where(pos, w * np.log(safe), 0.0)).sum(axis=-1)
    return np.log(np.where(pos, safe ** a, 0.0).sum(axis=-1)) / (1.0 - a)


def cap_cost(spectra, chi: int) -> np.ndarray:
    """What a bond cap at ``chi`` discards at each bond: eps_k(chi) = sum_{i >= chi} lambda_k[i] of descending Schmidt weights
    (``Context.bond_spectra`` with every weight, the default), shape ``spectra.shape[:-1]``.  For a normalised state
    ||psi - psi_chi||^2 <= 2 sum_k eps_k(chi).  ``chi`` must be >= 1."""
    if int(chi) != chi or int(chi) < 1:
        raise ValueError(f"chi must be an integer >= 1 (got {chi!r})")
    w = _spectra_array(spectra)
    return w[..., int(chi):][..., ::-1].sum(axis=-1)  # from the small end


def schmidt_rank(spectra, tol: float) -> np.ndarray:
    """Number of Schmidt weights above ``tol`` at each bond (weights below about 1e-15 are rounding noise of the environments)."""
    return np.count_nonzero(_spectra_array(spectra) > float(tol), axis=-1)


def _block_side(side) -> int:
    """'left' / 'right' -> 0 / 1; an int goes to the library as it is (which rejects anything but 0 and 1)."""
    if isinstance(side, str):
        if side not in ("left", "right"):
            raise ValueError(f"side must be 'left' or 'right', got {side!r}")
        return 0 if side == "left" else 1
    if isinstance(side, bool) or not isinstance(side, (int, np.integer)):
        raise ValueError(f"side must be 'left' or 'right', got {side!r}")
    return int(side)


def _block_widths(widths, n_sites: int) -> np.ndarray:
    """The width list as int32; ``None`` means 1 .. n_sites.  (The library rejects widths that are not strictly increasing in
    1 .. n_sites.)"""
    if widths is None:
        return np.arange(1, n_sites + 1, dtype=np.int32)
    w = np.asarray(widths)
    if w.ndim != 1 or (w.size and not np.issubdtype(w.dtype, np.integer)) or w.dtype == np.bool_:
        raise ValueError(f"widths must be a list of ints, got {widths!r}")
    return np.ascontiguousarray(w, dtype=np.int32)


def block_kernel(O, Sx, Sy=None, form: str = "rbf", gamma=None) -> np.ndarray:
    """A kernel from reduced-state overlaps (``Context.block_overlaps``), pure numpy.  ``O`` has shape (..., ny, nx), ``Sx`` (..., nx)
    and ``Sy`` (..., ny) the self overlaps (purities); ``Sy=None`` means Y is X.
        "overlap"     K = O
        "normalized"  K = O[j, i] / sqrt(Sx[i] Sy[j])   (nan where Sx[i] Sy[j] <= 0)
        "rbf"         K = exp(-gamma (Sx[i] + Sy[j] - 2 O[j, i])) = exp(-gamma ||rho_A(x_i) - rho_A(y_j)||_F^2), gamma > 0 (default 1)
    With ``Sy=None`` the result is exactly symmetric (the upper triangle is mirrored) and "normalized" and "rbf" have a diagonal of
    exactly 1.0.  Estimates from shots (``Context.shot_block_overlaps``) are taken as they are: an estimated purity can be <= 0, and
    "normalized" is then nan in that state's row and column, off the diagonal."""
    if form not in ("overlap", "normalized", "rbf"):
        raise ValueError(f"form must be 'overlap', 'normalized' or 'rbf', got {form!r}")
    g = 1.0 if gamma is None else float(gamma)
    if not (g > 0.0 and np.isfinite(g)):
        raise ValueError(f"gamma must be > 0 and finite, got {gamma!r}")
    O = np.asarray(O, dtype=np.float64)
    Sx = np.asarray(Sx, dtype=np.float64)
    sym = Sy is None
    Sy = Sx if sym else np.asarray(Sy, dtype=np.float64)
    if O.ndim < 2 or Sx.shape != O.shape[:-2] + O.shape[-1:] or Sy.shape != O.shape[:-2] + O.shape[-2:-1]:
        raise ValueError(f"O of shape {O.shape} needs Sx of shape (..., nx) and Sy of shape (..., ny), got {Sx.shape} and {Sy.shape}")
    if form == "overlap":
        K = O.copy()
    elif form == "normalized":
        with np.errstate(invalid="ignore", divide="ignore"):
            prod = Sx[..., None, :] * Sy[..., :, None]
            K = np.where(prod > 0.0, O / np.sqrt(np.where(prod > 0.0, prod, 1.0)), np.nan)
    else:
        K = np.exp(-g * ((Sx[..., None, :] + Sy[..., :, None]) - 2.0 * O))
    if sym:
        iu = np.triu_indices(O.shape[-1], 1)
        K[..., iu[1], iu[0]] = K[..., iu[0], iu[1]]
        if form != "overlap":
            d = np.arange(O.shape[-1])
            K[..., d, d] = 1.0
    return K


WINDOW_MAX_WIDTH = 6  # qubits of a window (qk_window_rdms_host)
_PAULI = np.array([[[1, 0], [0, 1]], [[0, 1], [1, 0]], [[0, -1j], [1j, 0]], [[1, 0], [0, -1]]], dtype=np.complex128)  # I, X, Y, Z


def _window_rdms(rho, name: str = "rho") -> tuple:
    """``rho`` as complex128 of shape (n_states, n_windows, D, D), D = 2^w, and w."""
    r = np.asarray(rho, dtype=np.complex128)
    D = r.shape[-1] if r.ndim == 4 else 0
    w = int(D).bit_length() - 1
    if r.ndim != 4 or r.shape[2] != D or D < 2 or (1 << w) != D or r.shape[1] < 1:
        raise ValueError(f"{name} must have shape (n_states, n_windows, 2^w, 2^w) with w >= 1, got {np.shape(rho)}")
    return r, w


def window_columns(rho) -> np.ndarray:
    """The real feature columns of window RDMs: (n_states, n_windows, D, D) complex -> (n_states, 2 n_windows D^2) float64, all real
    parts then all imaginary parts -- what ``projected_window_gram`` hands to ``feature_gram``."""
    r, _ = _window_rdms(rho)
    f = r.reshape(r.shape[0], -1)
    return np.ascontiguousarray(np.concatenate([f.real, f.imag], axis=1))


def window_overlaps(rx, ry=None):
    """``(O, Sx, Sy)`` from window RDMs (``Context.window_rdms``), pure numpy, in the conventions of ``Context.block_overlaps``:
    O[a, j, i] = tr(rho_a(x_i) rho_a(y_j)) = Re sum rho_a(x_i)[s][s'] conj(rho_a(y_j)[s][s']), shape (n_windows, ny, nx), rows = Y
    (or X), and the purities Sx (n_windows, nx), Sy (n_windows, ny) -- what ``block_kernel(O[a], Sx[a], Sy[a], form=...)`` takes per
    window.  A symmetric call (``ry=None``) computes the pairs i <= j, mirrors them, takes Sx from the diagonal and returns
    ``Sy = Sx``: O is exactly symmetric and its diagonal is the bits of Sx."""
    x, w = _window_rdms(rx, "rx")

    def planes(r):  # (n_windows, n_states, 2 D^2) real: the overlap is a dot product of these rows
        f = r.reshape(r.shape[0], r.shape[1], -1).transpose(1, 0, 2)
        return np.ascontiguousarray(np.concatenate([f.real, f.imag], axis=2))

    def purity(f):
        return np.einsum("asd,asd->as", f, f)

    fx = planes(x)
    if ry is None:
        O = np.einsum("ajd,aid->aji", fx, fx)
        iu = np.triu_indices(fx.shape[1], 1)
        O[:, iu[1], iu[0]] = O[:, iu[0], iu[1]]
        d = np.arange(fx.shape[1])
        Sx = purity(fx)
        O[:, d, d] = Sx
        return O, Sx, Sx
    y, wy = _window_rdms(ry, "ry")
    if wy != w or y.shape[1] != x.shape[1]:
        raise ValueError(f"Y RDMs of shape {y.shape} do not match X RDMs of shape {x.shape}")
    fy = planes(y)
    return np.einsum("ajd,aid->aji", fy, fx), purity(fx), purity(fy)


def rdm_paulis(rho) -> np.ndarray:
    """Pauli coefficients of w-qubit density matrices, pure numpy: ``rho`` of shape (..., 2^w, 2^w) gives float64 of shape
    (..., 4, ..., 4) with w axes of size 4, c[p_0 .. p_{w-1}] = tr(rho P_{p_0} (x) .. (x) P_{p_{w-1}}), P = (I, X, Y, Z), qubit 0 of
    the window the first of them -- the convention of ``local_pair_paulis``'s T[k][p][q], so rho = 2^-w sum c P (``paulis_rdm``).
    Real for a Hermitian rho (the imaginary part is dropped)."""
    r = np.asarray(rho, dtype=np.complex128)
    D = r.shape[-1] if r.ndim >= 2 else 0
    w = int(D).bit_length() - 1
    if r.ndim < 2 or r.shape[-2] != D or D < 2 or (1 << w) != D:
        raise ValueError(f"rho must have shape (..., 2^w, 2^w) with w >= 1, got {np.shape(rho)}")
    lead = r.shape[:-2]
    nl = len(lead)
    t = r.reshape(lead + (2,) * (2 * w))  # (.., s_0 .. s_{w-1}, s'_0 .. s'_{w-1})
    for j in range(w):
        # qubit j: its row axis s_j is nl + j (the axes before it are already p_0 .. p_{j-1}), its column axis s'_j is nl + w (the
        # first column axis left); c[p] = sum rho[s][s'] P_p[s'][s], and p goes where s_j was
        t = np.moveaxis(np.tensordot(t, _PAULI, axes=([nl + j, nl + w], [2, 1])), -1, nl + j)
    return np.ascontiguousarray(t.real)


def paulis_rdm(c, width=None) -> np.ndarray:
    """The inverse of ``rdm_paulis``: coefficients of shape (..., 4, ..., 4) give rho = 2^-w sum c[p_0 .. p_{w-1}] P_{p_0} (x) .. (x)
    P_{p_{w-1}}, complex128 of shape (..., 2^w, 2^w).  ``width=None`` takes every trailing axis of size 4 (at most 6) as a qubit;
    give ``width`` when a leading axis happens to have size 4."""
    t = np.asarray(c, dtype=np.float64)
    if width is None:
        w = 0
        while w < min(t.ndim, WINDOW_MAX_WIDTH) and t.shape[t.ndim - 1 - w] == 4:
            w += 1
    else:
        w = int(width)
    if w < 1 or w > t.ndim or t.shape[t.ndim - w:] != (4,) * w:
        raise ValueError(f"coefficients must have shape (..., 4, ..., 4) with w >= 1 trailing axes of size 4, got {np.shape(c)} (width {width!r})")
    nl = t.ndim - w
    t = t.astype(np.complex128)
    for j in range(w):  # the first coefficient axis left, p_j -> (s_j, s'_j) = P_p[s_j][s'_j], appended at the end
        t = np.tensordot(t, _PAULI, axes=([nl], [0]))
    order = list(range(nl)) + [nl + 2 * j for j in range(w)] + [nl + 2 * j + 1 for j in range(w)]  # rows, then columns
    D = 1 << w
    return np.ascontiguousarray(t.transpose(order).reshape(t.shape[:nl] + (D, D))) / D


def _string_table(n_sites: int, strings, checked: bool = True) -> np.ndarray:
    """``strings`` as the uint8 code table (m, n_sites): an integer array of that shape is taken as it is (``checked=False`` leaves
    codes of 4 .. 255 to the library), anything else goes through ``pauli_strings``."""
    if isinstance(strings, np.ndarray) and strings.ndim == 2:
        if strings.dtype.kind not in "iu" or strings.shape[0] < 1 or strings.shape[1] != n_sites:
            raise ValueError(f"strings must be an integer code table of shape (m >= 1, {n_sites}), got shape {strings.shape}, dtype {strings.dtype}")
        hi = 3 if checked else 255
        bad = np.flatnonzero(((strings < 0) | (strings > hi)).any(axis=1))
        if bad.size:
            raise ValueError(f"strings[{int(bad[0])}] holds a code outside 0..3 = I, X, Y, Z")
        return np.ascontiguousarray(strings, dtype=np.uint8)
    return pauli_strings(n_sites, strings)


def _string_tables(bits, bases):
    """(bits (ns, T, n), bases as given, per_state) of a shot-string call"""
    b = _shot_bits(bits, "bits")
    c = np.asarray(bases)
    if b.shape[0] < 1 or b.shape[1] < 1:
        raise ValueError(f"bits must hold at least one state and one shot, got shape {b.shape}")
    if c.dtype.kind not in "iu" or c.shape not in (b.shape[1:], b.shape):
        raise ValueError(f"bases must be an integer array of shape {b.shape[1:]} (shared) or {b.shape} (per state), got shape {c.shape}, dtype {c.dtype}")
    return b, c, int(c.ndim == 3)


def pack_string_words(strings) -> np.ndarray:
    """The packed record of every Pauli string of a code table (m, n_qubits), codes 0..3 = I, X, Y, Z: uint32 of shape
    (m, groups, 2) with groups = ceil(n / 32).  Bit k % 32 of group k // 32 holds ``code & 1`` (plane 0) and ``code >> 1`` (plane 1) of
    qubit k; I and the pad bits are 0 in both, so the OR of the planes is the string's support."""
    s = np.asarray(strings)
    if s.ndim != 2 or s.dtype.kind not in "iu" or s.shape[1] < 1 or s.shape[1] > SHADOW_MAX_QUBITS:
        raise ValueError(f"strings must be an integer code table (m, n_qubits <= {SHADOW_MAX_QUBITS}), got shape {s.shape}, dtype {s.dtype}")
    s = s.astype(np.int64)
    if s.size and (s.min() < 0 or s.max() > 3):
        raise ValueError("strings holds a code outside 0..3 = I, X, Y, Z")
    m, n = s.shape
    groups = (n + 31) // 32
    planes = np.zeros((m, groups * 32, 2), dtype=np.int64)
    planes[:, :n, 0], planes[:, :n, 1] = s & 1, s >> 1
    planes = planes.reshape(m, groups, 32, 2)
    return (planes << np.arange(32, dtype=np.int64)[:, None]).sum(axis=-2).astype(np.uint32)


def shot_string_sums(bits, bases, strings):
    """Pauli strings against measurement shots in plain numpy -- the mirror of ``Context.shot_string_sums_host``, the same integers
    from the packed records (``pack_shadow_words``, ``pack_string_words``) and ``_popcount32``: ``(sums, counts)``, both int64 of
    shape (n_states, m).  ``bits`` (n_states, shots, n) was measured in ``bases``, (shots, n) shared by every state or
    (n_states, shots, n) per state, codes 1, 2, 3 = X, Y, Z; ``strings`` is anything ``pauli_strings(n, ...)`` takes, or a code
    table (m, n).  A shot matches a string when its bases equal the string's codes on every qubit of the string's support;
        counts[s, m] = #{matching shots},   sums[s, m] = sum over them of prod_{k in support} (1 - 2 bits[s, t, k]).
    The all-identity string has counts = sums = shots.  Works in chunks: the temporaries stay at a few MiB."""
    b, c, per_state = _string_tables(bits, bases)
    ns, T, n = b.shape
    S = pack_string_words(_string_table(n, strings))  # (m, G, 2)
    m, G = S.shape[:2]
    supp = S[..., 0] | S[..., 1]
    sums, counts = np.zeros((ns, m), dtype=np.int64), np.zeros((ns, m), dtype=np.int64)
    t_rows = max(1, (1 << 14) // G)  # shots packed at a time
    for s in range(ns):
        for t0 in range(0, T, t_rows):
            r = pack_shadow_words(b[s, t0 : t0 + t_rows], c[s, t0 : t0 + t_rows] if per_state else c[t0 : t0 + t_rows])  # (t, G, 3)
            m_rows = max(1, (1 << 18) // (r.shape[0] * G))  # strings at a time
            for m0 in range(0, m, m_rows):
                s1, s2, sp = S[None, m0 : m0 + m_rows, :, 0], S[None, m0 : m0 + m_rows, :, 1], supp[None, m0 : m0 + m_rows]
                match = ~(sp & ((s1 ^ r[:, None, :, 1]) | (s2 ^ r[:, None, :, 2]))).any(axis=-1)
                odd = np.bitwise_xor.reduce(r[:, None, :, 0] & sp, axis=-1)
                sign = 1 - 2 * (_popcount32(odd) & 1)
                counts[s, m0 : m0 + m_rows] += match.sum(axis=0)
                sums[s, m0 : m0 + m_rows] += np.where(match, sign, 0).sum(axis=0)
    return sums, counts


def string_values(sums, counts) -> np.ndarray:
    """The estimates of ``shot_string_sums``: ``sums / counts`` as float64, and 0.0 where ``counts == 0`` (the convention of
    ``estimate_paulis``)."""
    s, c = np.asarray(sums), np.asarray(counts)
    if s.shape != c.shape or s.dtype.kind not in "iu" or c.dtype.kind not in "iu":
        raise ValueError(f"sums and counts must be integer arrays of one shape, got {s.shape} ({s.dtype}) and {c.shape} ({c.dtype})")
    return np.where(c > 0, s / np.maximum(c, 1), 0.0)


def _window_width(width, n: int) -> int:
    if isinstance(width, bool) or not isinstance(width, (int, np.integer)) or not 1 <= width <= min(int(n), WINDOW_MAX_WIDTH):
        raise ValueError(f"width must be an int in 1 .. min(n_qubits, {WINDOW_MAX_WIDTH}) = {min(int(n), WINDOW_MAX_WIDTH)}, got {width!r}")
    return int(width)


def window_strings(n_qubits: int, width: int, starts=None) -> np.ndarray:
    """The 4^width Pauli strings of every window of ``width`` contiguous qubits, as the code table uint8 (n_windows 4^width,
    n_qubits): windows in the order of ``Context.window_rdms`` (``starts=None``: every window 0 .. n - width; otherwise strictly
    increasing ints in that range), and inside a window the strings in the index order of ``rdm_paulis``, the window's first qubit
    first -- string p_0 4^(w-1) + .. + p_{w-1} has P_{p_j} on qubit start + j.  Values of these strings reshaped to
    ``(n_states, n_windows) + (4,) * width`` are what ``paulis_rdm(..., width=width)`` takes (give ``width``: with four windows the
    window axis would pass for a qubit)."""
    n = int(n_qubits)
    if n < 1:
        raise ValueError(f"n_qubits must be >= 1 (got {n_qubits!r})")
    w = _window_width(width, n)
    if starts is None:
        st = np.arange(n - w + 1)
    else:
        st = np.asarray(starts)
        if st.ndim != 1 or st.size < 1 or not np.issubdtype(st.dtype, np.integer) or st.dtype == np.bool_:
            raise ValueError(f"starts must be a non-empty list of ints, got {starts!r}")
        if st.min() < 0 or st.max() > n - w or (np.diff(st) <= 0).any():
            raise ValueError(f"starts must be strictly increasing in 0 .. n_qubits - width = {n - w}, got {starts!r}")
    codes = (np.arange(4 ** w)[:, None] >> (2 * (w - 1 - np.arange(w)))[None, :]) & 3  # (4^w, w): p_0 is the leading digit
    out = np.zeros((len(st), 4 ** w, n), dtype=np.uint8)
    for i, a in enumerate(st):
        out[i, :, int(a) : int(a) + w] = codes
    return out.reshape(len(st) * 4 ** w, n)


def estimate_window_rdms(bits, bases, width: int, starts=None, sums=shot_string_sums):
    """``Context.estimate_window_rdms`` with the integers from ``sums`` (the numpy mirror ``shot_string_sums`` unless the context
    passes its device call): ``(rho_hat, counts)``, documented there."""
    b = _shot_bits(bits, "bits")
    n = b.shape[2]
    w = _window_width(width, n)
    S = window_strings(n, w, starts)
    tot, counts = sums(b, bases, S)
    shape = (b.shape[0], S.shape[0] >> (2 * w)) + (4,) * w
    return paulis_rdm(string_values(tot, counts).reshape(shape), width=w), counts.reshape(shape)


def window_settings(shots: int, n_qubits: int, width: int) -> np.ndarray:
    """Designed measurement bases for the windows of ``width`` qubits: uint8 (shots, n_qubits), codes 1..3 = X, Y, Z.  Shot t uses
    setting ``t % 3^width``, and qubit k gets ``1 +`` digit number ``k % width`` of the setting in base 3.  The ``width`` qubits of
    any window have distinct residues, so they run through all 3^width basis choices together: every string of weight v >= 1 on any
    window of that width matches exactly ``shots / 3^v`` shots when 3^width divides ``shots``."""
    if isinstance(shots, bool) or not isinstance(shots, (int, np.integer)) or shots < 1:
        raise ValueError(f"shots must be an int >= 1 (got {shots!r})")
    n = int(n_qubits)
    if n < 1:
        raise ValueError(f"n_qubits must be >= 1 (got {n_qubits!r})")
    w = _window_width(width, n)
    setting = np.arange(int(shots)) % 3 ** w
    digit = np.arange(n) % w
    return (1 + (setting[:, None] // 3 ** digit[None, :]) % 3).astype(np.uint8)


def _dims_table(states) -> np.ndarray:
    return np.ascontiguousarray(np.stack([np.asarray(m.bond_dims(), dtype=np.int32) for m in states]))


def pack_state(mps, layout=QK_LAYOUT_LPR):
    """Host-only: the padded split-plane image of one MPS and its per-site offsets."""
    L = lib()
    dims = np.ascontiguousarray(mps.bond_dims(), dtype=np.int32)
    n = len(mps)
    tens = [np.ascontiguousarray(t, dtype=np.complex128) for t in mps.tensors]
    ptrs = (C.c_void_p * n)(*[t.ctypes.data for t in tens])
    size = L.qk_pack_state_size(n, dims.ctypes.data)
    out = np.empty(size, dtype=np.float64)
    offs = np.empty(n, dtype=np.int64)
    _check(L.qk_pack_state(n, dims.ctypes.data, ptrs, layout, out.ctypes.data, offs.ctypes.data), "qk_pack_state")
    return out, offs


def unpack_state(planes, dims, offsets) -> list:
    """Host-only, pure numpy, the inverse of ``pack_state``: the site tensors ``[left bond, 2, right bond]`` (complex128) of one
    state from a padded split-plane image.  ``planes``: the doubles of the image; ``dims``: the state's true bonds chi[0..n];
    ``offsets``: the re-plane offset of every site in doubles (the im plane follows its re plane)."""
    planes = np.asarray(planes, dtype=np.float64).reshape(-1)
    dims = [int(d) for d in np.asarray(dims).reshape(-1)]
    offsets = [int(o) for o in np.asarray(offsets).reshape(-1)]
    if len(offsets) != len(dims) - 1:
        raise ValueError(f"{len(dims)} bond dimensions need {len(dims) - 1} site offsets, got {len(offsets)}")
    tensors = []
    for k, off in enumerate(offsets):
        l, r = dims[k], dims[k + 1]
        pl, pr = (l + 15) // 16 * 16, (r + 15) // 16 * 16
        plane = pl * 2 * pr
        if l < 1 or r < 1 or off < 0 or off + 2 * plane > planes.size:
            raise ValueError(f"site {k}: bonds ({l}, {r}) at offset {off} do not lie inside an image of {planes.size} doubles")
        re = planes[off : off + plane].reshape(pl, 2, pr)[:l, :, :r]
        im = planes[off + plane : off + 2 * plane].reshape(pl, 2, pr)[:l, :, :r]
        tensors.append(re + 1j * im)
    return tensors


class Plan:
    """Ordered share of the Gram's (x, y) pairs for one rank (host object)."""

    def __init__(self, x_dims, y_dims=None, world_size=1, rank=0, block=0, quads=False, orient=None):
        L = lib()
        xd = np.ascontiguousarray(x_dims, dtype=np.int32)
        self.symmetric = y_dims is None
        yd = None if self.symmetric else np.ascontiguousarray(y_dims, dtype=np.int32)
        self.nx = xd.shape[0]
        self.ny = self.nx if self.symmetric else yd.shape[0]
        n_sites = xd.shape[1] - 1
        if orient is None:  # default: on (QK_PLAN_ORIENT=0 lists every pair of a symmetric plan as i <= j)
            orient = os.environ.get("QK_PLAN_ORIENT", "1") != "0"
        self.orient = bool(orient) and self.symmetric and not quads
        h = _P()
        _check(
            L.qk_plan_create(
                n_sites, self.nx, xd.ctypes.data, self.ny, None if yd is None else yd.ctypes.data,
                (QK_PLAN_SYMMETRIC if self.symmetric else 0) | (QK_PLAN_QUADS if quads else 0) | (QK_PLAN_ORIENT if self.orient else 0), world_size, rank, block, C.byref(h),
            ),
            "qk_plan_create",
        )
        self._h = h
        self.world_size, self.rank, self.quads = world_size, rank, bool(quads)

    @classmethod
    def create_all(cls, x_dims, y_dims=None, world_size=1):
        """The plans of all ``world_size`` ranks from ONE cost pass (``qk_plan_create_all``): equal to ``[Plan(x_dims, y_dims,
        world_size, r) for r in range(world_size)]`` at a fraction of the host time."""
        xd = np.ascontiguousarray(x_dims, dtype=np.int32)
        sym = y_dims is None
        yd = None if sym else np.ascontiguousarray(y_dims, dtype=np.int32)
        orient = sym and os.environ.get("QK_PLAN_ORIENT", "1") != "0"
        out = (_P * int(world_size))()
        _check(lib().qk_plan_create_all(xd.shape[1] - 1, xd.shape[0], xd.ctypes.data, xd.shape[0] if sym else yd.shape[0], None if sym else yd.ctypes.data,
                                        (QK_PLAN_SYMMETRIC if sym else 0) | (QK_PLAN_ORIENT if orient else 0), int(world_size), out), "qk_plan_create_all")
        plans = []
        for r in range(int(world_size)):
            p = cls.__new__(cls)
            p.symmetric, p.nx, p.ny = sym, xd.shape[0], xd.shape[0] if sym else yd.shape[0]
            p.orient, p._h, p.world_size, p.rank, p.quads = orient, _P(out[r]), int(world_size), r, False
            plans.append(p)
        return plans

    @property
    def handle(self):
        return self._h

    @property
    def num_pairs(self) -> int:
        return int(lib().qk_plan_num_pairs(self._h))

    @property
    def total_pairs(self) -> int:
        return int(lib().qk_plan_total_pairs(self._h))

    @property
    def max_pairs_per_rank(self) -> int:
        return int(lib().qk_plan_max_pairs_per_rank(self._h))

    def pairs(self) -> np.ndarray:
        n = self.num_pairs
        if n == 0:
            return np.zeros((0, 2), dtype=np.int32)
        ptr = lib().qk_plan_pairs(self._h)
        buf = (C.c_int32 * (2 * n)).from_address(ptr)
        return np.frombuffer(buf, dtype=np.int32).reshape(n, 2).copy()

    @property
    def first_run(self) -> int:
        """Pairs [first_run, num_pairs) are the run the site-fused sweep takes with its two-workgroups-per-CU shape."""
        return int(lib().qk_plan_first_run(self._h))

    def cost(self) -> dict:
        """Host cost of making this plan and the tile-reuse lower bound on its bytes (qk_plan_cost)."""
        ms, th, tr = C.c_double(0), C.c_int32(0), C.c_double(0)
        _check(lib().qk_plan_cost(self._h, C.byref(ms), C.byref(th), C.byref(tr)), "qk_plan_cost")
        return {"plan_ms": ms.value, "threads": int(th.value), "tile_reuse_bytes": tr.value}

    @property
    def edge_sites(self) -> int:
        """Sites at either end of the chain that the site-fused sweep takes from the sets' edge blocks (0: none)."""
        return int(lib().qk_plan_edge_sites(self._h))

    def queues(self):
        """(number of device work queues, qstart[17]): queue s = pairs [qstart[s], qstart[s+1]) -- 8 per run of the list, one
        per XCD (include/qkgram.h: qk_plan_queues); 1 queue = the flat cost-ordered list."""
        qs = np.zeros(17, dtype=np.int64)
        return int(lib().qk_plan_queues(self._h, qs.ctypes.data)), qs

    def stats(self) -> dict:
        st = QkStats()
        _check(lib().qk_plan_stats(self._h, C.byref(st)), "qk_plan_stats")
        return st.as_dict()

    def close(self):
        if self._h:
            lib().qk_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MpsSet:
    """Device-resident list of MPS (opaque handle)."""

    def __init__(self, ctx, handle, dims):
        self.ctx, self._h, self.dims = ctx, handle, dims
        ctx._adopt(self)  # the context closes the sets that are still alive before it goes (their handles point into it)

    @property
    def handle(self):
        return self._h

    def __len__(self):
        return self.dims.shape[0]

    def info(self) -> dict:
        a, b, c, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        _check(lib().qk_mps_set_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)), "qk_mps_set_info")
        return {"n_states": a.value, "n_sites": b.value, "max_padded_bond": c.value, "device_bytes": d.value}

    def image(self):
        """The fp64 device image of the set: (number of doubles, device address of the planes, true bonds
        [n_states, n_sites + 1], re-plane offsets in doubles [n_states, n_sites])."""
        n, ptr = C.c_int64(), _P()
        ns, nsites = self.dims.shape[0], self.dims.shape[1] - 1
        dims = np.zeros((ns, nsites + 1), dtype=np.int32)
        offs = np.zeros((ns, nsites), dtype=np.int64)
        _check(lib().qk_mps_set_image(self._h, C.byref(n), C.byref(ptr), dims.ctypes.data, offs.ctypes.data), "qk_mps_set_image")
        return int(n.value), int(ptr.value or 0), dims, offs

    def copy_image(self, dst_ptr: int, n_doubles: int):
        """Copy the planes into a device or host buffer of ``n_doubles`` doubles (the send buffer of the all-gather)."""
        _check(lib().qk_mps_set_copy_image(self._h, _P(dst_ptr), int(n_doubles)), "qk_mps_set_copy_image")

    def download(self) -> list:
        """The states of an fp64 set back on the host, as ``list[MPS]``: the true-bond corners of the device image."""
        from .mps import MPS

        n_doubles, _, dims, offs = self.image()
        planes = np.empty(n_doubles, dtype=np.float64)
        self.copy_image(planes.ctypes.data, n_doubles)
        return [MPS(unpack_state(planes, dims[s], offs[s])) for s in range(dims.shape[0])]

    @property
    def precision(self) -> int:
        """Bits of a real of the device image: 64 (complex128) or 32 (complex64)."""
        return int(lib().qk_mps_set_precision(self._h))

    @property
    def centre(self) -> int:
        """The orthogonality centre the set records: the common centre of a snapshot of the device builder (``BuiltScan.set``,
        ``build_mps_set``, ``build_share``), -1 where the gauge is unknown -- an uploaded, gathered, converted or compressed set."""
        return int(lib().qk_mps_set_centre(self._h))

    def to_f32(self) -> "MpsSet":
        """A complex64 copy of this set on the same device; sweeps over fp32 sets run the
        fp32-MFMA kernel.  Both sets of a Gram must have the same precision."""
        h = _P()
        _check(lib().qk_mps_set_to_f32(self.ctx.handle, self._h, C.byref(h)), "qk_mps_set_to_f32")
        return MpsSet(self.ctx, h, self.dims)

    def close(self):
        if self._h:
            lib().qk_mps_set_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _GateProgram:
    """The circuits of one device-builder call as the arrays of a ``qk_program``: the shared gate structure (``op``, ``q0`` and,
    with a matrix table, ``mat``), the per-state angles, and the matrix table of op codes 8 and 9 -- shared (stride 0) when every
    circuit's ``mats`` is the same array bit for bit, otherwise stacked per state (stride n_mats).  ``QkError`` when the circuits do
    not share their gate structure.  The table goes to the C entry as it is: it validates indices and unitarity.

    The channel tables (op codes 10 and 11) belong to the gate structure: ``channel``, ``kraus`` and ``n_kraus``, ``kraus2`` and
    ``n_kraus2`` must be the same for every circuit; ``branch`` may differ per state (one row for all when they agree, stride 0, otherwise a row per state).  ``seed``,
    ``state_index`` and ``trajectory`` (a scalar for all states, or one per state; ``None``: 0 .. n-1 and 0) name the trajectories,
    ``first_gate`` the position of the first gate in the uninterrupted program.  The condition rows ``cond_gate`` and ``cond_mask``
    are gate structure too: the same for every circuit."""

    def __init__(self, what, circuits, seed=0, state_index=None, trajectory=None, first_gate=0):
        c0 = circuits[0]
        self.what = what
        self.n, self.ns = int(c0.n_qubits), len(circuits)
        self.op = np.ascontiguousarray(c0.op, dtype=np.int8)
        self.q0 = np.ascontiguousarray(c0.q0, dtype=np.int32)
        with_table = getattr(c0, "mats", None) is not None and getattr(c0, "mat", None) is not None
        for c in circuits[1:]:
            same = c.n_qubits == c0.n_qubits and np.array_equal(c.op, c0.op) and np.array_equal(c.q0, c0.q0)
            has = getattr(c, "mats", None) is not None and getattr(c, "mat", None) is not None
            if same and (has != with_table or (has and not (np.array_equal(c.mat, c0.mat) and np.shape(c.mats) == np.shape(c0.mats)))):
                same = False
            if not same:
                raise QkError(f"{what}: the circuits of one call must share their gate structure")
        self.alpha = np.ascontiguousarray(np.stack([np.asarray(c.alpha, dtype=np.float64) for c in circuits]))
        self.n_mats, self.stride, self.mats, self.mat = 0, 0, None, None
        if with_table:
            m0 = np.asarray(c0.mats)
            if m0.ndim != 3 or m0.shape[1:] != (4, 4) or np.shape(c0.mat) != self.op.shape:
                raise QkError(f"{what}: the matrix table must be [n_mats][4][4] with one index per gate, got shapes {m0.shape} and {np.shape(c0.mat)}")
            self.n_mats = int(m0.shape[0])
            self.mat = np.ascontiguousarray(c0.mat, dtype=np.int32)
            tables = [np.ascontiguousarray(c.mats, dtype=np.complex128) for c in circuits]
            if all(t is tables[0] or t.tobytes() == tables[0].tobytes() for t in tables[1:]):
                self.mats = tables[0]
            else:
                self.mats, self.stride = np.ascontiguousarray(np.stack(tables)), self.n_mats
        self.n_channels, self.bstride, self.kraus, self.n_kraus, self.channel, self.branch = 0, 0, None, None, None, None
        self.n_channels2, self.kraus2, self.n_kraus2 = 0, None, None

        def table(c, d):  # the table of d x d channels of circuit c: (kraus, n_kraus) or None
            k, nk = (getattr(c, "kraus", None), getattr(c, "n_kraus", None)) if d == 2 else (getattr(c, "kraus2", None), getattr(c, "n_kraus2", None))
            return None if k is None or nk is None or getattr(c, "channel", None) is None else (np.ascontiguousarray(k, dtype=np.complex128), nk)

        for d in (2, 4):
            tabs = [table(c, d) for c in circuits]
            if not any(t is not None for t in tabs):
                continue
            code = 10 if d == 2 else 11
            t0 = tabs[0]
            for c, t in zip(circuits, tabs):
                if t is None or t0 is None or t[0].shape != t0[0].shape or not (np.array_equal(c.channel, c0.channel) and np.array_equal(t[1], t0[1])
                                                                                 and t[0].tobytes() == t0[0].tobytes()):
                    raise QkError(f"{what}: the circuits of one call must share their gate structure (the channels of op code {code} and their table included)")
            k0 = t0[0]
            if k0.ndim != 4 or k0.shape[1:] != (d * d, d, d) or np.shape(t0[1]) != k0.shape[:1] or np.shape(c0.channel) != self.op.shape:
                raise QkError(f"{what}: the {'two-qubit ' if d == 4 else ''}channel table must be [n_channels][{d * d}][{d}][{d}] with a count per channel and a channel per gate, "
                              f"got shapes {k0.shape}, {np.shape(t0[1])} and {np.shape(c0.channel)}")
            if d == 2:
                self.n_channels, self.kraus, self.n_kraus = int(k0.shape[0]), k0, np.ascontiguousarray(t0[1], dtype=np.int32)
            else:
                self.n_channels2, self.kraus2, self.n_kraus2 = int(k0.shape[0]), k0, np.ascontiguousarray(t0[1], dtype=np.int32)
        if self.n_channels or self.n_channels2:
            self.channel = np.ascontiguousarray(c0.channel, dtype=np.int32)
            rows = [np.full(self.op.shape, -1, dtype=np.int32) if c.branch is None else np.ascontiguousarray(c.branch, dtype=np.int32) for c in circuits]
            if any(r.shape != self.op.shape for r in rows):
                raise QkError(f"{what}: branch must hold one entry per gate of the program")
            if all(np.array_equal(r, rows[0]) for r in rows[1:]):
                self.branch = rows[0]
            else:
                self.branch, self.bstride = np.ascontiguousarray(np.stack(rows)), int(self.op.shape[0])
        self.cond_gate, self.cond_mask = None, None
        conds = [(getattr(c, "cond_gate", None), getattr(c, "cond_mask", None)) for c in circuits]
        if any(g is not None for g, _ in conds):
            g0, m0 = conds[0]
            same = lambda a, b: (a is None) == (b is None) and (a is None or np.array_equal(a, b))  # noqa: E731
            if not all(same(g, g0) and same(m, m0) for g, m in conds[1:]):
                raise QkError(f"{what}: the circuits of one call must share their gate structure (the condition rows included)")
            if np.shape(g0) != self.op.shape or (m0 is not None and np.shape(m0) != self.op.shape):
                raise QkError(f"{what}: cond_gate and cond_mask must hold one entry per gate, got shapes {np.shape(g0)}, {np.shape(m0)}")
            self.cond_gate = np.ascontiguousarray(g0, dtype=np.int32)  # the C entry validates the rows
            self.cond_mask = None if m0 is None else np.ascontiguousarray(np.asarray(m0).astype(np.uint32))
        self.seed = int(_seed_key(seed)[0]) | (int(_seed_key(seed)[1]) << 32)
        self.state_index = self._ids("state_index", state_index, np.arange(self.ns))
        self.trajectory = self._ids("trajectory", trajectory, np.zeros(self.ns, dtype=np.int64))
        if isinstance(first_gate, bool) or not isinstance(first_gate, (int, np.integer)) or not 0 <= int(first_gate) < 1 << 32:
            raise ValueError(f"first_gate must be an int in 0 .. 2^32 - 1 (got {first_gate!r})")
        self.first_gate = int(first_gate)

    def _ids(self, name, v, default):
        a = np.asarray(default if v is None else v)
        if a.ndim == 0:
            a = np.full(self.ns, a)
        if a.shape != (self.ns,) or a.dtype.kind not in "iu" or a.min() < 0 or a.max() >= 1 << 32:
            raise ValueError(f"{name} must be an int or one int per state ({self.ns}) in 0 .. 2^32 - 1, got {v!r}")
        return np.ascontiguousarray(a, dtype=np.uint32)

    def build(self, ctx, truncation_fidelity, value_of_zero, max_bond, flags, cps=None, src=None, src_j=0):
        """One launch of the device builder: the handle of the built states (``qk_built``)."""
        tables = {}
        if self.op.shape[0]:  # an empty program has no gate that reads a table or a condition: it is built as a plain one
            tables = dict(mats=self.mats, mat=self.mat, mats_state_stride=self.stride, kraus=self.kraus, n_kraus=self.n_kraus, kraus2=self.kraus2, n_kraus2=self.n_kraus2,
                          channel=self.channel, branch=self.branch, branch_state_stride=self.bstride, cond_gate=self.cond_gate, cond_mask=self.cond_mask)
        prog = _program.fill_program(self.ns, self.n, self.op, self.q0, self.alpha, seed=self.seed, state_index=self.state_index, trajectory=self.trajectory,
                                     first_gate=self.first_gate, **tables)
        run = _program.sized(_program.QkBuildRun, flags=flags, trunc_budget=max(0.0, 1.0 - float(truncation_fidelity)), value_of_zero=float(value_of_zero), max_bond=int(max_bond),
                             n_checkpoints=0 if cps is None else int(cps.shape[0]), checkpoints=None if cps is None else cps.ctypes.data, initial=src, initial_snapshot=src_j)
        h = _P()
        _check(lib().qk_build_program(ctx._h, C.byref(prog), C.byref(run), C.byref(h)), "qk_build_program")
        return h


def _built_trajectories(h, ns, j=-1):
    """``(logw float64 (ns,), branches int8 (ns, n_channel_gates))`` of a built handle: the log-weights at snapshot j (-1: the last)
    and the branch every channel gate of the program took (-1 where a dropped state stopped early)."""
    if j < 0:
        j += int(lib().qk_built_num_snapshots(h))
    logw = np.zeros(ns, dtype=np.float64)
    _check(lib().qk_built_logw_at(h, j, logw.ctypes.data), "qk_built_logw_at")
    nk = int(lib().qk_built_num_channel_gates(h))
    branches = np.full((ns, nk), -1, dtype=np.int8)
    if nk:
        _check(lib().qk_built_branches(h, branches.ctypes.data), "qk_built_branches")
    return logw, branches


def _built_launch(h) -> dict:
    """What the builder launched for a built handle: {"grid": workgroups, "threads": threads of each, "slots": workgroups per CU x
    CUs, what the grid was clipped to}.  grid == slots < n_states: workgroups took more than one state."""
    g, t, sl = C.c_int32(), C.c_int32(), C.c_int32()
    _check(lib().qk_built_launch(h, C.byref(g), C.byref(t), C.byref(sl)), "qk_built_launch")
    return {"grid": int(g.value), "threads": int(t.value), "slots": int(sl.value)}


class BuiltScan:
    """The snapshots of ``Context.build_mps_scan``: owns the builder's handle (one device heap with every snapshot of every state)
    until ``close()``; a context manager.  ``checkpoints[j]`` gates were done at snapshot j; the last snapshot is the finished
    circuit.  ``set(j)`` / ``states(j)`` are independent of the scan afterwards."""

    def __init__(self, ctx, handle, n_states, n_qubits, kgate_at=None):
        self.ctx, self._h, self.n_states, self.n_qubits = ctx, handle, int(n_states), int(n_qubits)
        self._kgate_at = kgate_at  # positions of the channel gates in the program: a snapshot's states carry the branches taken so far
        ns = int(lib().qk_built_num_snapshots(handle))
        cps = np.zeros(ns, dtype=np.int32)
        _check(lib().qk_built_checkpoints(handle, cps.ctypes.data), "qk_built_checkpoints")
        self.checkpoints = [int(c) for c in cps]
        ms = C.c_double()
        _check(lib().qk_built_info(handle, None, None, None, None, C.byref(ms)), "qk_built_info")
        self.kernel_ms = ms.value
        self.launch = _built_launch(handle)  # {"grid", "threads", "slots"} of the scan's one launch
        self.first_gate = 0  # position of the program's first gate in the uninterrupted circuit (build_mps_scan sets it)
        self._norms = None  # Context.seed: the norm every state came with
        ctx._adopt(self)  # closed with the context: the heap lives on its device

    @property
    def handle(self):
        return self._h

    def __len__(self):
        return len(self.checkpoints)

    def _index(self, j) -> int:
        if self._h is None:
            raise QkError("the scan is closed")
        k = int(j)
        if k < 0:
            k += len(self.checkpoints)
        if not 0 <= k < len(self.checkpoints):
            raise IndexError(f"snapshot {j!r} outside 0 .. {len(self.checkpoints) - 1}")
        return k

    def _info(self, j):
        j = self._index(j)
        dims = np.zeros((self.n_states, self.n_qubits + 1), dtype=np.int32)
        fid = np.zeros(self.n_states, dtype=np.float64)
        offs = np.zeros(self.n_states, dtype=np.int64)
        centre = np.zeros(self.n_states, dtype=np.int32)
        total = C.c_int64()
        _check(lib().qk_built_info_at(self._h, j, dims.ctypes.data, fid.ctypes.data, offs.ctypes.data, centre.ctypes.data, C.byref(total)), "qk_built_info_at")
        return j, dims, fid, offs, centre, int(total.value)

    def info(self, j) -> dict:
        """Snapshot j: {"dims": bond tables (n_states, n_qubits + 1), "fidelity": the fidelity product so far (n_states,),
        "centre": site of the orthogonality centre (n_states,), "heap_bytes": bytes of the snapshot's tensors in the heap,
        "logw": the log-weights of the trajectories so far (n_states,), "branches": the branch of every channel gate of the whole
        program (n_states, n_channel_gates), whichever snapshot is asked, "grid", "threads", "slots": the scan's launch}."""
        k, dims, fid, _, centre, total = self._info(j)
        logw, branches = _built_trajectories(self._h, self.n_states, k)
        seed = {} if self._norms is None else {"norm": self._norms.copy()}  # a seed (``Context.seed``): the norms the states came with
        return {"dims": dims, "fidelity": fid, "centre": centre, "heap_bytes": 16 * total, "logw": logw, "branches": branches, **seed, **self.launch}

    def set(self, j) -> "MpsSet":
        """Snapshot j as a device-resident set (packed on the device: nothing is downloaded); feeds ``gram``, ``local_paulis``,
        ``compress`` ... like any set."""
        j, dims, *_ = self._info(j)
        hs = _P()
        _check(lib().qk_mps_set_from_built_at(self.ctx.handle, self._h, j, C.byref(hs)), "qk_mps_set_from_built_at")
        return MpsSet(self.ctx, hs, dims)

    def states(self, j) -> list:
        """Snapshot j on the host: ``list[MPS]``, each with its fidelity so far."""
        from .mps import MPS

        j, dims, fid, _, _, total = self._info(j)
        logw, branches = _built_trajectories(self._h, self.n_states, j)
        done = np.count_nonzero(np.asarray(self._kgate_at) < self.checkpoints[j]) if self._kgate_at is not None else branches.shape[1]
        flat = np.empty(max(total, 1), dtype=np.complex128)
        _check(lib().qk_built_download_at(self._h, j, flat.ctypes.data), "qk_built_download_at")
        out, pos = [], 0
        for s_ in range(self.n_states):
            tensors = []
            for k in range(self.n_qubits):
                sz = int(dims[s_, k]) * 2 * int(dims[s_, k + 1])
                tensors.append(flat[pos : pos + sz].reshape(int(dims[s_, k]), 2, int(dims[s_, k + 1])).copy())
                pos += sz
            out.append(MPS(tensors, float(fid[s_]), float(logw[s_]), branches[s_, :done]))
        return out

    def close(self):
        if self._h:
            lib().qk_built_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One engine context per device (what ``CuTensorNetHandle(device_id)`` is to the reference,
    /root/reference/gpu_backend/kernel_state_ansatz.py:213)."""

    def __init__(self, device_id: int = 0):
        h = _P()
        _check(lib().qk_ctx_create(int(device_id), C.byref(h)), "qk_ctx_create")
        self._h, self.device_id = h, int(device_id)
        self._sets = weakref.WeakSet()

    def _adopt(self, mps_set):
        if not hasattr(self, "_sets"):
            self._sets = weakref.WeakSet()
        self._sets.add(mps_set)

    def _close_sets(self):
        """Destroy every MpsSet made on this context that is still alive: ``qk_mps_set_destroy`` dereferences the set's context,
        so a set must never outlive it (a later ``close()`` / ``__del__`` of such a set is then a no-op)."""
        for s in list(getattr(self, "_sets", ())):
            s.close()

    @property
    def handle(self):
        return self._h

    def set_stream(self, hip_stream: int | None):
        """Use exactly this hipStream_t (0 = HIP's null stream = torch's default stream); ``None``
        goes back to the context's private stream."""
        if hip_stream is None:
            _check(lib().qk_ctx_use_own_stream(self._h), "qk_ctx_use_own_stream")
        else:
            _check(lib().qk_ctx_set_stream(self._h, _P(int(hip_stream))), "qk_ctx_set_stream")

    def synchronize(self):
        _check(lib().qk_ctx_synchronize(self._h), "qk_ctx_synchronize")

    def trim(self):
        """Release the device memory the context keeps between calls (sweep scratch, the device builder's arena and workspace)."""
        _check(lib().qk_ctx_trim(self._h), "qk_ctx_trim")

    def debug_mma_bench(self, which, wgs_per_cu, reps=2000):
        out = C.c_double()
        _check(lib().qk_debug_mma_bench(self._h, which, wgs_per_cu, reps, C.byref(out)), "qk_debug_mma_bench")
        return out.value

    def debug_profile(self):
        out = (C.c_uint64 * 8)()
        _check(lib().qk_debug_profile(self._h, out), "qk_debug_profile")
        return list(out)

    def selftest(self):
        _check(lib().qk_selftest_mfma(self._h), "qk_selftest_mfma")

    def debug_jacobi(self, a):
        """The device builder's one-sided Jacobi on one matrix: returns (A V, V, column norms, order by decreasing norm)."""
        a = np.array(a, dtype=np.complex128, order="C")
        p, q = a.shape
        v = np.zeros((q, q), dtype=np.complex128)
        sig = np.zeros(q, dtype=np.float64)
        order = np.zeros(q, dtype=np.int32)
        _check(lib().qk_debug_jacobi(self._h, p, q, a.ctypes.data, v.ctypes.data, sig.ctypes.data, order.ctypes.data), "qk_debug_jacobi")
        return a, v, sig, order

    def debug_jacobi_precond(self, a):
        """The builder's preconditioned block factorisation on one matrix (p x q, 16 <= q): (W = A V, V, sig, ord, sweeps, ms)."""
        a = np.ascontiguousarray(a, dtype=np.complex128).copy()
        p, q = a.shape
        v = np.zeros((q, q), dtype=np.complex128)
        sig = np.zeros(q, dtype=np.float64)
        ord_ = np.zeros(q, dtype=np.int32)
        st = np.zeros(6, dtype=np.int32)
        _check(lib().qk_debug_jacobi_precond(self._h, p, q, a.ctypes.data, v.ctypes.data, sig.ctypes.data, ord_.ctypes.data, st.ctypes.data), "qk_debug_jacobi_precond")
        self.last_precond_ms = [float(np.uint32(t)) / 1e5 for t in st[1:]]  # all, sort + copy, Gram-Schmidt, sweeps, V and W = A V
        return a, v, sig, ord_, int(st[0]), self.last_precond_ms[0]

    def seed(self, xs, index=None, value_of_zero: float = 1e-16, sweep: bool = False) -> BuiltScan:
        """Given states as the starting point of a build: a ``BuiltScan`` with ONE snapshot of zero gates (``.checkpoints == [0]``)
        that every build call resumes from through ``initial=(seed, 0)``.  ``xs`` is a device-resident ``MpsSet`` of this context
        (fp64) or a ``list[MPS]`` (uploaded for the call).  ``index[s]`` names the state of ``xs`` that build state s starts from
        (``None``: one build state per state of ``xs``): the heap holds each state once, so one state may start many circuits
        (broadcast) or T trajectories.

        A set that records its centre (``MpsSet.centre >= 0``: a snapshot of the device builder) is taken verbatim, bit for bit,
        with fidelity 1 -- unless ``sweep`` asks for the other path.  Every other set may be in any gauge and of any norm (bonds up
        to 512): after a finite check it goes through the canonical sweep of ``compress(xs, max_discard=0)`` (a bond whose rank is
        below its dimension shrinks to its rank), the centre ends on the last site and is divided by its norm.  ``info(0)`` carries
        ``norm`` (per build state: the norm the state came with; 1 on the verbatim path), ``fidelity``, ``centre`` and ``dims``.
        ``QkError`` naming the state for a state of norm 0 or with an entry that is not finite.  Close it, or use ``with``."""
        from .mps import MPS

        own = None
        if isinstance(xs, MPS):
            xs = [xs]
        if not isinstance(xs, MpsSet):
            own = xs = self.upload(list(xs))
        try:
            ns_set, n = xs.dims.shape[0], xs.dims.shape[1] - 1
            idx = None
            if index is not None:
                idx = np.asarray(index)
                if idx.ndim != 1 or idx.dtype.kind not in "iu" or idx.shape[0] < 1:
                    raise ValueError(f"index must be a non-empty 1-D array of ints, got {index!r}")
                idx = np.ascontiguousarray(idx, dtype=np.int32)
            n_states = ns_set if idx is None else int(idx.shape[0])
            norms, fid = np.zeros(ns_set, dtype=np.float64), np.zeros(ns_set, dtype=np.float64)
            h = _P()
            _check(lib().qk_built_from_set(self._h, xs.handle, n_states, None if idx is None else idx.ctypes.data, float(value_of_zero), 1 if sweep else 0, C.byref(h),
                                           norms.ctypes.data, fid.ctypes.data), "qk_built_from_set")
        finally:
            if own is not None:
                own.close()
        scan = BuiltScan(self, h, n_states, n)
        scan._norms = norms if idx is None else norms[idx]
        return scan

    def _resume(self, what, initial, ns, initial_index, value_of_zero):
        """What ``initial=`` of a build call means: ``(seed to close or None, handle, snapshot, first gate)``.  ``(scan, j)`` is a
        snapshot of an earlier scan; an ``MpsSet``, a ``list[MPS]`` or one ``MPS`` (for all ``ns`` states) is seeded for the call,
        with ``initial_index`` as the ``index`` of ``seed``."""
        from .mps import MPS

        if initial is None:
            if initial_index is not None:
                raise ValueError(f"{what}: initial_index goes with initial states")
            return None, None, 0, 0
        if isinstance(initial, tuple) and len(initial) == 2 and isinstance(initial[0], BuiltScan):
            if initial_index is not None:
                raise ValueError(f"{what}: initial_index goes with given states, not with a snapshot (seed them with Context.seed(xs, index))")
            scan, j = initial
            k = scan._index(j)
            return None, scan.handle, k, scan.first_gate + scan.checkpoints[k]
        if isinstance(initial, MPS):
            if initial_index is not None:
                raise ValueError(f"{what}: one initial MPS starts every state; initial_index goes with a set or a list")
            initial, initial_index = [initial], np.zeros(ns, dtype=np.int32)
        if not isinstance(initial, MpsSet) and not (isinstance(initial, (list, tuple)) and len(initial) and all(isinstance(m, MPS) for m in initial)):
            raise ValueError(f"{what}: initial must be (BuiltScan, snapshot index), an MpsSet, a list of MPS or one MPS, got {initial!r}")
        seed = self.seed(initial, initial_index, value_of_zero)
        if seed.n_states != ns:
            seed.close()
            raise ValueError(f"{what}: the initial states start {seed.n_states} builds, the call has {ns} circuits")
        return seed, seed.handle, 0, 0

    def _build_from(self, what, circuits, seed, state_index, trajectory, truncation_fidelity, value_of_zero, max_bond, flags, initial, initial_index):
        """One launch of a one-snapshot build call, from |0...0> or from ``initial``: ``(built handle, gate program)``."""
        own, src, src_j, base = self._resume(what, initial, len(circuits), initial_index, value_of_zero)
        try:
            prog = _GateProgram(what, circuits, seed, state_index, trajectory, base)
            cps = None if src is None else np.array([int(prog.op.shape[0])], dtype=np.int32)  # a resumed build goes through the scan entries
            return prog.build(self, truncation_fidelity, value_of_zero, max_bond, flags, cps, src, src_j), prog
        finally:
            if own is not None:
                own.close()

    def build_mps(self, circuits, truncation_fidelity: float = 1.0 - 1e-16, value_of_zero: float = 1e-16, max_bond: int = 256, partial: bool = False, truncate: bool = False,
                  seed=0, state_index=None, trajectory=None, initial=None, initial_index=None):
        """Device MPS builder (/root/reference/gpu_backend/kernel_state_ansatz.py:221, 263): the MPS of every
        bound circuit of the list (``ansatz.BoundCircuit``; they must share one gate structure, as the data points of one
        ansatz do) in ONE launch.  Returns (list[MPS], info) with info = {"kernel_ms", "total_complex", "dropped", and the launch:
        "grid" workgroups of "threads" threads, clipped to "slots" = workgroups per CU x CUs}.  With
        ``partial`` a state that outgrows ``max_bond`` does not fail the call: its entry in the list is ``None`` and its index is
        in info["dropped"] (build it with the host builder).

        Circuits with Kraus channels (op code 10) are run as quantum trajectories: state s draws its branches from ``seed``,
        ``state_index[s]`` and ``trajectory[s]`` (an int for all, or one per state; ``None``: 0 .. n-1 and 0; see
        ``channel_uniform``), so its result does not depend on what else the call builds.  info["logw"] (n,) and info["branches"]
        (n, n_channel_gates) record the log-probability and the branches; the states carry them too.

        ``initial`` / ``initial_index``: the circuits are applied to given states instead of |0...0>, as in ``build_mps_scan``."""
        from .mps import MPS

        circuits = list(circuits)
        if not circuits:
            raise QkError("build_mps needs at least one circuit")
        h, prog = self._build_from("build_mps", circuits, seed, state_index, trajectory, truncation_fidelity, value_of_zero, max_bond,
                                   (1 if partial else 0) | (2 if truncate else 0), initial, initial_index)
        n, ns = prog.n, prog.ns
        try:
            dims = np.zeros((ns, n + 1), dtype=np.int32)
            fid = np.zeros(ns, dtype=np.float64)
            offs = np.zeros(ns, dtype=np.int64)
            total, ms = C.c_int64(), C.c_double()
            _check(lib().qk_built_info(h, dims.ctypes.data, fid.ctypes.data, offs.ctypes.data, C.byref(total), C.byref(ms)), "qk_built_info")
            flat = np.empty(total.value, dtype=np.complex128)
            _check(lib().qk_built_download(h, flat.ctypes.data), "qk_built_download")
            logw, branches = _built_trajectories(h, ns)
            launch = _built_launch(h)
        finally:
            lib().qk_built_destroy(h)
        states, dropped = [], []
        for s_ in range(ns):
            if fid[s_] < 0:
                states.append(None)
                dropped.append(s_)
                continue
            pos, tensors = int(offs[s_]), []
            for k in range(n):
                sz = int(dims[s_, k]) * 2 * int(dims[s_, k + 1])
                tensors.append(flat[pos : pos + sz].reshape(int(dims[s_, k]), 2, int(dims[s_, k + 1])))
                pos += sz
            states.append(MPS(tensors, float(fid[s_]), float(logw[s_]), branches[s_]))
        return states, {"kernel_ms": ms.value, "total_complex": int(total.value), "dropped": dropped, "logw": logw, "branches": branches, **launch}

    def build_mps_set(self, circuits, truncation_fidelity: float = 1.0 - 1e-16, value_of_zero: float = 1e-16, max_bond: int = 256, truncate: bool = False, seed=0,
                      state_index=None, trajectory=None, initial=None, initial_index=None):
        """Like ``build_mps`` but the states never leave the device: returns (MpsSet, info) with info = {"kernel_ms", "dims",
        "fidelity", "logw", "branches", "grid", "threads", "slots"}; the set feeds ``gram`` / ``gram_values`` directly."""
        circuits = list(circuits)
        if not circuits:
            raise QkError("build_mps_set needs at least one circuit")
        h, prog = self._build_from("build_mps_set", circuits, seed, state_index, trajectory, truncation_fidelity, value_of_zero, max_bond, 2 if truncate else 0, initial,
                                   initial_index)
        n, ns = prog.n, prog.ns
        hs = _P()
        try:
            dims = np.zeros((ns, n + 1), dtype=np.int32)
            fid = np.zeros(ns, dtype=np.float64)
            ms = C.c_double()
            _check(lib().qk_built_info(h, dims.ctypes.data, fid.ctypes.data, None, None, C.byref(ms)), "qk_built_info")
            logw, branches = _built_trajectories(h, ns)
            launch = _built_launch(h)
            _check(lib().qk_mps_set_from_built(self._h, h, C.byref(hs)), "qk_mps_set_from_built")
        finally:
            lib().qk_built_destroy(h)
        return MpsSet(self, hs, dims), {"kernel_ms": ms.value, "dims": dims, "fidelity": fid, "logw": logw, "branches": branches, **launch}

    def build_mps_scan(self, circuits, checkpoints, truncation_fidelity: float = 1.0 - 1e-16, value_of_zero: float = 1e-16, max_bond: int = 256, truncate: bool = False,
                       initial=None, partial: bool = False, seed=0, state_index=None, trajectory=None, first_gate=None, initial_index=None) -> BuiltScan:
        """``build_mps_set`` that also keeps every state after ``checkpoints[j]`` gates (gate counts: strictly increasing, in
        1 .. n_gates, the last one n_gates; ``KernelStateAnsatz.layer_ends()`` for a scan over depth): ONE launch, the snapshots are
        copies and the run does the arithmetic of a run without them, so the last snapshot is what ``build_mps`` returns.  Returns a
        ``BuiltScan`` (``.checkpoints``, ``.kernel_ms``, ``.info(j)``, ``.set(j)``, ``.states(j)``; close it, or use ``with``).  A
        snapshot is in mixed-canonical gauge; all snapshots share one device heap.

        ``initial=(scan, j)`` resumes: the states start as snapshot j of an earlier scan of this context (same number of states and
        qubits, no bond above ``max_bond``) and ``circuits`` are the gates that follow it -- ``c.sliced(scan.checkpoints[j],
        c.n_gates)`` continues the same circuits, gate for gate the arithmetic of the uninterrupted run.  ``scan`` is left untouched.
        ``initial`` may also be given states -- an ``MpsSet``, a ``list[MPS]`` (one per circuit, or picked by ``initial_index`` as
        the ``index`` of ``Context.seed``) or one ``MPS`` for all circuits: they are seeded by ``Context.seed`` for the call.
        ``ValueError`` for bad checkpoints; ``partial`` goes with one checkpoint and no ``initial`` only (``QkError`` otherwise).

        ``seed``, ``state_index`` and ``trajectory`` name the trajectories of circuits with Kraus channels as in ``build_mps``.
        ``first_gate`` is the position of the first gate of ``circuits`` in the uninterrupted program; ``None`` takes it from
        ``initial`` (``scan.checkpoints[j]`` plus the ``first_gate`` that scan was given; 0 without one), so a resumed build draws
        what the uninterrupted run draws and its log-weights go on from the snapshot's.  ``info(j)`` and ``states(j)`` carry
        ``logw`` and ``branches``."""
        from .ansatz import check_checkpoints

        circuits = list(circuits)
        if not circuits:
            raise QkError("build_mps_scan needs at least one circuit")
        cps = np.ascontiguousarray(check_checkpoints(checkpoints, int(np.shape(circuits[0].op)[0])), dtype=np.int32)
        own, src, src_j, base = self._resume("build_mps_scan", initial, len(circuits), initial_index, value_of_zero)
        try:
            prog = _GateProgram("build_mps_scan", circuits, seed, state_index, trajectory, base if first_gate is None else first_gate)
            n, ns = prog.n, prog.ns
            h = prog.build(self, truncation_fidelity, value_of_zero, max_bond, (1 if partial else 0) | (2 if truncate else 0), cps, src, src_j)
        finally:
            if own is not None:
                own.close()
        scan = BuiltScan(self, h, ns, n, np.flatnonzero((prog.op == 10) | (prog.op == 11)) if prog.n_channels or prog.n_channels2 else None)
        scan.first_gate = prog.first_gate
        return scan

    def set_from_packed(self, dims_true, offsets, planes_ptr: int, n_doubles: int) -> MpsSet:
        """A set assembled from packed images (``MpsSet.image`` of several ranks, gathered into one buffer on the device or
        on the host): see ``qk_mps_set_from_packed``."""
        dims = np.ascontiguousarray(dims_true, dtype=np.int32)
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        h = _P()
        _check(lib().qk_mps_set_from_packed(self._h, dims.shape[0], dims.shape[1] - 1, dims.ctypes.data, offs.ctypes.data, _P(planes_ptr), int(n_doubles), C.byref(h)),
               "qk_mps_set_from_packed")
        return MpsSet(self, h, dims)

    def build_share(self, circuits, truncation_fidelity: float = 1.0 - 1e-16, value_of_zero: float = 1e-16, max_bond: int = 256, partial: bool = False, truncate: bool = False,
                    seed=0, state_index=None, trajectory=None, initial=None, initial_index=None):
        """Device builder for one rank's share of a data set, the states staying on the device whenever possible: returns
        (MpsSet, None, info) when every state fitted ``max_bond`` (packed on the device by ``qk_mps_set_from_built``: nothing
        is downloaded), else (None, list[MPS | None], info) with the dropped states ``None`` (``partial`` only), to be
        completed by the host builder.  info = {"kernel_ms", "dims", "fidelity", "dropped", "logw", "branches", "grid", "threads", "slots"}; ``seed``,
        ``state_index`` and ``trajectory`` as in ``build_mps``."""
        from .mps import MPS

        circuits = list(circuits)
        if not circuits:
            raise QkError("build_share needs at least one circuit")
        h, prog = self._build_from("build_share", circuits, seed, state_index, trajectory, truncation_fidelity, value_of_zero, max_bond,
                                   (1 if partial else 0) | (2 if truncate else 0), initial, initial_index)
        n, ns = prog.n, prog.ns
        try:
            dims = np.zeros((ns, n + 1), dtype=np.int32)
            fid = np.zeros(ns, dtype=np.float64)
            offs = np.zeros(ns, dtype=np.int64)
            total, ms = C.c_int64(), C.c_double()
            _check(lib().qk_built_info(h, dims.ctypes.data, fid.ctypes.data, offs.ctypes.data, C.byref(total), C.byref(ms)), "qk_built_info")
            dropped = [int(k) for k in np.nonzero(fid < 0)[0]]
            logw, branches = _built_trajectories(h, ns)
            info = {"kernel_ms": ms.value, "dims": dims, "fidelity": fid, "dropped": dropped, "logw": logw, "branches": branches, **_built_launch(h)}
            if not dropped:
                hs = _P()
                _check(lib().qk_mps_set_from_built(self._h, h, C.byref(hs)), "qk_mps_set_from_built")
                return MpsSet(self, hs, dims), None, info
            flat = np.empty(total.value, dtype=np.complex128)
            _check(lib().qk_built_download(h, flat.ctypes.data), "qk_built_download")
        finally:
            lib().qk_built_destroy(h)
        states = []
        for s_ in range(ns):
            if fid[s_] < 0:
                states.append(None)
                continue
            pos, tensors = int(offs[s_]), []
            for k in range(n):
                sz = int(dims[s_, k]) * 2 * int(dims[s_, k + 1])
                tensors.append(flat[pos : pos + sz].reshape(int(dims[s_, k]), 2, int(dims[s_, k + 1])))
                pos += sz
            states.append(MPS(tensors, float(fid[s_]), float(logw[s_]), branches[s_]))
        return None, states, info

    def upload(self, states, layout=QK_LAYOUT_LPR) -> MpsSet:
        states = list(states)
        if not states:
            raise QkError("cannot upload an empty list of MPS")
        n_sites = len(states[0])
        if any(len(m) != n_sites for m in states):
            raise QkError("all MPS of a set must have the same number of sites")
        dims = _dims_table(states)
        keep = [[np.ascontiguousarray(t, dtype=np.complex128) for t in m.tensors] for m in states]
        flat = [t.ctypes.data for ts in keep for t in ts]
        ptrs = (C.c_void_p * len(flat))(*flat)
        h = _P()
        _check(
            lib().qk_mps_set_create(self._h, len(states), n_sites, dims.ctypes.data, ptrs, layout, C.byref(h)),
            "qk_mps_set_create",
        )
        return MpsSet(self, h, dims)

    def gram_values(self, xset: MpsSet, yset: MpsSet | None, plan: Plan, values_ptr: int, z_ptr: int | None = None):
        """Asynchronous: enqueue the sweep of ``plan``'s pairs; device pointers are plain addresses."""
        _check(
            lib().qk_gram_values(self._h, xset.handle, None if yset is None else yset.handle, plan.handle, _P(values_ptr), _P(z_ptr) if z_ptr else None),
            "qk_gram_values",
        )

    def gram_values_host(self, xset: MpsSet, yset: MpsSet | None, plan: Plan, want_z: bool = False):
        """Synchronous sweep of ``plan``'s pairs; returns |z|^2 (and z if asked) as host arrays."""
        n = plan.num_pairs
        vals = np.zeros(n, dtype=np.float64)
        z = np.zeros((n, 2), dtype=np.float64) if want_z else None
        _check(
            lib().qk_gram_values_host(self._h, xset.handle, None if yset is None else yset.handle, plan.handle,
                                      vals.ctypes.data, None if z is None else z.ctypes.data),
            "qk_gram_values_host",
        )
        return (vals, z[:, 0] + 1j * z[:, 1]) if want_z else vals

    def scatter(self, pairs_ptr: int, values_ptr: int, n: int, k_ptr: int, ld: int, mirror: bool):
        _check(lib().qk_scatter(self._h, _P(pairs_ptr), _P(values_ptr), int(n), _P(k_ptr), int(ld), 1 if mirror else 0), "qk_scatter")

    def gram(self, xset: MpsSet, yset: MpsSet | None = None) -> np.ndarray:
        """Synchronous whole Gram: rows = Y (or X), cols = X."""
        nx = len(xset)
        ny = nx if yset is None else len(yset)
        out = np.zeros((ny, nx), dtype=np.float64)
        _check(lib().qk_gram_host(self._h, xset.handle, None if yset is None else yset.handle, out.ctypes.data, nx), "qk_gram_host")
        return out

    def overlaps(self, xset: MpsSet, yset: MpsSet | None = None) -> np.ndarray:
        """Synchronous complex overlaps z[j, i] = <x_i|y_j>."""
        nx = len(xset)
        ny = nx if yset is None else len(yset)
        out = np.zeros((ny, nx, 2), dtype=np.float64)
        _check(lib().qk_overlaps_host(self._h, xset.handle, None if yset is None else yset.handle, out.ctypes.data), "qk_overlaps_host")
        return out[..., 0] + 1j * out[..., 1]

    def local_paulis(self, mps_set: MpsSet, norms: bool = False):
        """Bloch vectors of every state of an fp64 set: F[state, k] = (<X_k>, <Y_k>, <Z_k>) of qubit k, float64 of shape
        (n_states, n_sites, 3); with ``norms=True`` also <psi|psi> of each state, as ``(F, norms)``.  Synchronous."""
        info = mps_set.info()
        F = np.zeros((info["n_states"], info["n_sites"], 3), dtype=np.float64)
        nrm = np.zeros(info["n_states"], dtype=np.float64)
        _check(lib().qk_local_paulis_host(self._h, mps_set.handle, F.ctypes.data, nrm.ctypes.data), "qk_local_paulis_host")
        return (F, nrm) if norms else F

    def projected_gram(self, fx, fy=None, gamma=None) -> np.ndarray:
        """Projected quantum kernel K[j, i] = exp(-gamma/2 sum_k |Fx[i, k] - Fy[j, k]|^2) of Bloch vectors (``local_paulis``):
        shape (ny, nx), rows = Y (or X).  ``gamma=None`` means 1 / n_sites.  Synchronous."""
        fx = np.ascontiguousarray(fx, dtype=np.float64)
        if fx.ndim != 3 or fx.shape[2] != 3:
            raise ValueError(f"features must have shape (n_states, n_sites, 3), got {fx.shape}")
        nx, n = fx.shape[0], fx.shape[1]
        g = projected_gamma(gamma, n)
        if fy is not None:
            fy = np.ascontiguousarray(fy, dtype=np.float64)
            if fy.ndim != 3 or fy.shape[1:] != fx.shape[1:]:
                raise ValueError(f"Y features of shape {fy.shape} do not match X features of shape {fx.shape}")
        ny = nx if fy is None else fy.shape[0]
        out = np.zeros((ny, nx), dtype=np.float64)
        _check(lib().qk_projected_gram_host(self._h, n, nx, fx.ctypes.data, ny, None if fy is None else fy.ctypes.data, g, out.ctypes.data, nx),
               "qk_projected_gram_host")
        return out

    def local_pair_paulis(self, mps_set: MpsSet, singles: bool = False, norms: bool = False, max_dist: int = 1):
        """Pauli correlators of neighbouring qubits of every state of an fp64 set: T[state, k, p, q] = <P_p on qubit k, P_q on
        qubit k+1>, P = (I, X, Y, Z), float64 of shape (n_states, n_sites - 1, 4, 4) -- the two-qubit reduced density matrix of the
        pair is 1/4 sum T[p, q] P_p (x) P_q.  ``singles=True`` adds the Bloch vectors and ``norms=True`` <psi|psi>, both the bits
        ``local_paulis`` returns: the result is ``T``, or the tuple ``(T[, F][, norms])``.  Synchronous.

        ``max_dist=D`` (1 <= D <= n_sites - 1) takes every pair (k, k+d), d = 1 .. D, in the order of ``pair_table(n_sites, D)``:
        T has shape (n_states, n_pairs, 4, 4), and its first n_sites - 1 rows are the bits of ``max_dist=1``."""
        info = mps_set.info()
        ns, n = info["n_states"], info["n_sites"]
        D = int(max_dist)
        n_pairs = D * n - D * (D + 1) // 2 if 1 <= D <= n - 1 else max(0, n - 1)  # (the library rejects a bad max_dist)
        T = np.zeros((ns, n_pairs, 4, 4), dtype=np.float64)
        F = np.zeros((ns, n, 3), dtype=np.float64) if singles else None
        nrm = np.zeros(ns, dtype=np.float64) if norms else None
        if D == 1:
            _check(lib().qk_local_pair_paulis_host(self._h, mps_set.handle, T.ctypes.data, None if F is None else F.ctypes.data,
                                                   None if nrm is None else nrm.ctypes.data), "qk_local_pair_paulis_host")
        else:
            _check(lib().qk_local_pair_paulis_dist_host(self._h, mps_set.handle, D, T.ctypes.data, None if F is None else F.ctypes.data,
                                                        None if nrm is None else nrm.ctypes.data), "qk_local_pair_paulis_dist_host")
        out = (T,) + ((F,) if singles else ()) + ((nrm,) if norms else ())
        return out if len(out) > 1 else T

    def projected_pair_gram(self, tx, ty=None, gamma=None, max_dist: int = 1) -> np.ndarray:
        """Two-qubit projected quantum kernel K[j, i] = exp(-gamma/4 sum_k sum_pq (Tx[i, k, p, q] - Ty[j, k, p, q])^2) of Pauli
        correlators (``local_pair_paulis``): shape (ny, nx), rows = Y (or X).  ``gamma=None`` means 1 / n_sites.  Synchronous.

        ``max_dist=D`` is the kernel over the pairs up to distance D (features of ``local_pair_paulis(max_dist=D)``): n_sites is
        inferred from n_pairs = D n - D (D + 1) / 2, and ``gamma=None`` means 1 / (n_sites D)."""
        tx = np.ascontiguousarray(tx, dtype=np.float64)
        if tx.ndim != 4 or tx.shape[1] < 1 or tx.shape[2:] != (4, 4):
            raise ValueError(f"features must have shape (n_states, n_sites - 1, 4, 4), got {tx.shape}")
        D = int(max_dist)
        nx, n = tx.shape[0], _pair_sites(tx.shape[1], D)
        if n is None:
            raise ValueError(f"features of shape {tx.shape} are not (n_states, n_pairs, 4, 4) of any chain with pairs up to max_dist {max_dist!r}")
        g = projected_gamma(gamma, n * D)
        if ty is not None:
            ty = np.ascontiguousarray(ty, dtype=np.float64)
            if ty.ndim != 4 or ty.shape[1:] != tx.shape[1:]:
                raise ValueError(f"Y features of shape {ty.shape} do not match X features of shape {tx.shape}")
        ny = nx if ty is None else ty.shape[0]
        out = np.zeros((ny, nx), dtype=np.float64)
        if D == 1:
            _check(lib().qk_projected_pair_gram_host(self._h, n, nx, tx.ctypes.data, ny, None if ty is None else ty.ctypes.data, g, out.ctypes.data, nx),
                   "qk_projected_pair_gram_host")
        else:
            _check(lib().qk_projected_pair_gram_dist_host(self._h, n, D, nx, tx.ctypes.data, ny, None if ty is None else ty.ctypes.data, g,
                                                          out.ctypes.data, nx), "qk_projected_pair_gram_dist_host")
        return out

    def pauli_expectations(self, mps_set: MpsSet, strings, norms: bool = False):
        """Expectation values <psi|P|psi> / <psi|psi> of Pauli strings for every state of an fp64 set: float64 of shape (n_states, m),
        column j the j-th string; with ``norms=True`` also <psi|psi> of each state (the bits of ``local_paulis``), as ``(V, norms)``.
        ``strings`` is anything ``pauli_strings(n_sites, ...)`` takes.  A string costs work on its support only; a value is the same
        bits whatever the other states and strings of the call.  Synchronous."""
        info = mps_set.info()
        ns, n = info["n_states"], info["n_sites"]
        S = pauli_strings(n, strings)
        V = np.zeros((ns, S.shape[0]), dtype=np.float64)
        nrm = np.zeros(ns, dtype=np.float64)
        _check(lib().qk_pauli_strings_host(self._h, mps_set.handle, S.shape[0], S.ctypes.data, V.ctypes.data, nrm.ctypes.data), "qk_pauli_strings_host")
        return (V, nrm) if norms else V

    def operator_expectations(self, xs: MpsSet, strings, ops=None, norms: bool = False):
        """Expectation values ``<psi| O_0 (x) ... (x) O_{n-1} |psi> / <psi|psi>`` of strings of single-site operators for every
        state of an fp64 set: complex128 of shape (n_states, m), column j the j-th string; with ``norms=True`` also <psi|psi> of
        each state (the bits of ``local_paulis``), as ``(V, norms)``.  ``strings`` and ``ops`` are what
        ``operator_strings(n_sites, strings, ops)`` takes: specs ``(names, qubits)`` over ``LOCAL_OPS`` and a dict of 2 x 2
        matrices, or rows of codes into a table ``ops`` of shape (n_ops, 2, 2) (code c = ``ops[c - 1]``, 0 = identity).  The
        operators need not be Hermitian.  A string costs the work of a Pauli string of the same support; an all-identity row is
        exactly 1 + 0j; a value is the same bits whatever the other states, strings and operators of the call.  Synchronous."""
        info = xs.info()
        ns, n = info["n_states"], info["n_sites"]
        table, codes = operator_strings(n, strings, ops)
        planes = np.ascontiguousarray(table).view(np.float64)
        V = np.zeros((ns, codes.shape[0], 2), dtype=np.float64)
        nrm = np.zeros(ns, dtype=np.float64)
        _check(lib().qk_operator_strings_host(self._h, xs.handle, table.shape[0], planes.ctypes.data, codes.shape[0], codes.ctypes.data, V.ctypes.data,
                                               nrm.ctypes.data), "qk_operator_strings_host")
        V = V[..., 0] + 1j * V[..., 1]
        return (V, nrm) if norms else V

    def mpo_expectations(self, xs: MpsSet, mpos, norms: bool = False):
        """Expectation values ``<psi| H_m |psi> / <psi|psi>`` of matrix-product operators (``Mpo``: sums of operator strings, see
        ``mpo_from_terms``, ``mpo_exponential``, ``mpo_product``) for every state of an fp64 set: complex128 of shape (n_states,
        n_mpos); with ``norms=True`` also <psi|psi> of each state (the bits of ``local_paulis``), as ``(V, norms)``.  One sweep
        over an MPO's support costs about its bond times one operator string of that support, whatever the number of terms.  An
        MPO whose tensors are all the 1 x 1 identity is exactly 1 + 0j; a bond-1 MPO gives the bits of its operator string; a value
        is the same bits whatever the other states and MPOs of the call.  Synchronous."""
        info = xs.info()
        ns, n = info["n_states"], info["n_sites"]
        ms = _mpo_list(mpos, n)
        bonds = np.ascontiguousarray(np.stack([m.bonds for m in ms]), dtype=np.int32)
        planes = np.ascontiguousarray(np.concatenate([m.packed() for m in ms]))
        V = np.zeros((ns, len(ms), 2), dtype=np.float64)
        nrm = np.zeros(ns, dtype=np.float64)
        _check(lib().qk_mpo_expectations_host(self._h, xs.handle, len(ms), bonds.ctypes.data, planes.ctypes.data, V.ctypes.data, nrm.ctypes.data),
               "qk_mpo_expectations_host")
        V = V[..., 0] + 1j * V[..., 1]
        return (V, nrm) if norms else V

    def apply_mpo(self, xs: MpsSet, mpo, max_bond: int | None = None, max_discard: float | None = None, value_of_zero: float = 1e-16, info: bool = False):
        """A new fp64 set with ``O|psi>`` for every state of ``xs`` and one ``Mpo`` (the device twin of ``MPS.apply_mpo``): true
        bonds ``w_k chi_k``, site ``B_k[(u, a)][s'][(v, b)] = sum_s W_k[u][v][s'][s] A_k[a][s][b]`` (row ``u chi_k + a``, column
        ``v chi_{k+1} + b``), general gauge (``centre`` = -1), not normalised; ``xs`` is left untouched.  With neither ``max_bond``
        nor ``max_discard`` the exact product is returned; a product bond above 512 is an error.  Otherwise the product goes
        through ``compress(max_bond, max_discard or 0, value_of_zero)`` and is closed.  ``info=True`` returns ``(set, info)`` with
        the product's bond table as ``product_bond_dims`` and, where it was compressed, ``compress``'s info.  A state's product is
        the same bits whatever the other states of the set.  Synchronous."""
        if not isinstance(mpo, Mpo):
            raise ValueError(f"apply_mpo takes one Mpo, got {type(mpo).__name__}")
        st = xs.info()
        ns, n = st["n_states"], st["n_sites"]
        if mpo.n_sites != n:
            raise ValueError(f"the Mpo has {mpo.n_sites} sites, the states have {n}")
        bonds = np.ascontiguousarray(mpo.bonds, dtype=np.int32)
        planes = np.ascontiguousarray(mpo.packed())
        h = _P()
        _check(lib().qk_mps_set_apply_mpo(self._h, xs.handle, bonds.ctypes.data, planes.ctypes.data, C.byref(h)), "qk_mps_set_apply_mpo")
        out = MpsSet(self, h, np.zeros((ns, n + 1), dtype=np.int32))
        out.dims = out.image()[2]
        extra = {"product_bond_dims": out.dims.copy()}
        if max_bond is not None or max_discard is not None:
            try:
                res = self.compress(out, max_bond, 0.0 if max_discard is None else max_discard, value_of_zero, info=True)
            finally:
                out.close()
            out = res[0]
            extra.update(res[1])
        return (out, extra) if info else out

    def operator_matrix(self, xs: MpsSet, mpo, ys: MpsSet | None = None, **compress_args) -> np.ndarray:
        """``M[j][i] = <y_j| O |x_i>``, complex128 of shape (len(ys or xs), len(xs)), not normalised: the Hamiltonian and overlap
        matrices of subspace methods, the off-diagonal partner of ``mpo_expectations``.  The MPO acts on the ket side, on ``xs``
        (one ``apply_mpo(xs, mpo, **compress_args)``); the conjugate is taken on ``ys`` by one ``overlaps(ys, O xs)``, whose
        ``z[i][j] = <y_j|O x_i>`` is returned transposed.  For ``<y|O^dagger|x>`` pass ``mpo.dagger()``.  Synchronous."""
        if "info" in compress_args:
            raise ValueError("operator_matrix returns the matrix alone: info is not an argument")
        ox = self.apply_mpo(xs, mpo, **compress_args)
        try:
            return np.ascontiguousarray(self.overlaps(xs if ys is None else ys, ox).T)
        finally:
            ox.close()

    def marginals(self, xs: MpsSet, bits, bases):
        """Probabilities of partial outcomes for every state of an fp64 set, the unmeasured qubits traced out: float64 of shape
        (n_states, n_strings).  ``bits`` is (n_strings, n_sites) of 0 / 1 (bit 0 = eigenvalue +1, as in ``sample``); ``bases`` is
        (n_strings, n_sites), or one row shared by every string, of codes 0..3: 0 = not measured (the bit there is ignored), 1,
        2, 3 = measured in X, Y, Z.  The result is the real part of the projector string (``operator_expectations`` with
        ``marginal_strings``) and is not clipped: a probability of exactly 0 may come out as rounding noise of either sign.  A
        row with no measured qubit is exactly 1.0.  Synchronous."""
        n = xs.info()["n_sites"]
        table, codes = marginal_strings(bits, bases, n)
        return np.ascontiguousarray(self.operator_expectations(xs, codes, ops=table).real)

    def sample(self, xs: MpsSet, shots: int, bases=None, seed: int = 0, first_state: int = 0, logp: bool = False):
        """Measurement shots of every state of an fp64 set, by perfect sampling along the chain: ``bits``, uint8 of shape
        (n_states, shots, n_sites), bit 0 = eigenvalue +1 of the Pauli the qubit was measured in.  ``bases`` is anything
        ``bases_table`` takes (``None``: all Z; a string such as ``"ZZXY"`` or a row shared by every shot; an array (shots, n_sites)
        of codes 1..3 = X, Y, Z, as ``random_bases`` makes).  With ``logp=True`` also the log of the exact probability of each
        drawn string in its bases, float64 (n_states, shots), as ``(bits, logp)``.  The uniforms are ``sample_uniform(seed,
        first_state + s, shot, site)``: the bits of a (state, shot) depend only on the seed, the state's global index, the shot, that
        shot's bases and the state's tensors -- the first shots of a longer call are the shorter call, and a share of a data set
        sampled with its offset as ``first_state`` gives the bits of the whole.  Synchronous."""
        info = xs.info()
        ns, n = info["n_states"], info["n_sites"]
        if isinstance(shots, bool) or not isinstance(shots, (int, np.integer)):
            raise ValueError(f"shots must be an int >= 1 (got {shots!r})")
        S = int(shots)
        B = None if bases is None else bases_table(bases, max(S, 0), n)
        key = _seed_key(seed)
        bits = np.zeros((ns, max(S, 0), n), dtype=np.uint8)
        lp = np.zeros((ns, max(S, 0)), dtype=np.float64)
        _check(lib().qk_sample_host(self._h, xs.handle, S, None if B is None else B.ctypes.data, int(key[0]) | (int(key[1]) << 32), int(first_state),
                                    bits.ctypes.data, lp.ctypes.data), "qk_sample_host")
        return (bits, lp) if logp else bits

    def amplitudes(self, xs: MpsSet, bits, bases=None, per_state: bool = False, logp: bool = False, scaled: bool = False, norms: bool = False):
        """Amplitudes ``<b| U_bases |psi_s>`` of given outcome strings under every state of an fp64 set -- strings the library did
        not draw, such as shots measured on hardware: complex128 of shape (n_states, n_strings).  ``bits`` is (n_strings, n_sites)
        of 0 / 1, shared by every state, or with ``per_state=True`` (n_states, n_strings, n_sites), a table per state (the bits
        ``sample`` returns); ``bases`` is anything ``bases_table`` takes, shared by every state (``None``: all Z; bit 0 = eigenvalue
        +1).  The device returns a mantissa and a power of two per amplitude (``MPS.amplitude`` is the mirror of its loop); the
        default result is ``ldexp(mant, expo)``, which may underflow to 0 for long or unnormalised chains -- ``scaled=True``
        returns ``(mant complex128, expo int32)`` instead, the larger component of ``mant`` in [0.5, 1).  ``logp=True`` appends
        the log of the probability ``|amplitude|^2 / <psi|psi>`` (-inf for a zero amplitude), float64 (n_states, n_strings), and
        ``norms=True`` <psi|psi> of each state (the bits of ``local_paulis``).  A (state, string) value is the same bits whatever
        the other states and strings, their order, the table's form and the run.  Synchronous."""
        info = xs.info()
        ns, n = info["n_states"], info["n_sites"]
        b = np.asarray(bits)
        want = 3 if per_state else 2
        if b.dtype.kind not in "iub" or b.ndim != want or b.shape[-1] != n or (per_state and b.shape[0] != ns):
            shape = f"({ns}, n_strings, {n})" if per_state else f"(n_strings, {n})"
            raise ValueError(f"bits must be an integer array of shape {shape}; got shape {b.shape}, dtype {b.dtype}")
        if b.size and (b.min() < 0 or b.max() > 255):
            raise ValueError(f"bits holds a value that is not 0 or 1 ({int(b.min() if b.min() < 0 else b.max())})")
        b = np.ascontiguousarray(b, dtype=np.uint8)
        S = b.shape[-2]
        B = None if bases is None else bases_table(bases, S, n)
        mant = np.zeros((ns, S, 2), dtype=np.float64)
        expo = np.zeros((ns, S), dtype=np.int32)
        lp = np.zeros((ns, S), dtype=np.float64) if logp else None
        nrm = np.zeros(ns, dtype=np.float64) if norms else None
        _check(lib().qk_amplitudes_host(self._h, xs.handle, S, b.ctypes.data, 1 if per_state else 0, None if B is None else B.ctypes.data, mant.ctypes.data,
                                        expo.ctypes.data, None if lp is None else lp.ctypes.data, None if nrm is None else nrm.ctypes.data), "qk_amplitudes_host")
        m = mant[..., 0] + 1j * mant[..., 1]
        out = ((m, expo) if scaled else (np.ldexp(mant[..., 0], expo) + 1j * np.ldexp(mant[..., 1], expo),)) + ((lp,) if logp else ()) + ((nrm,) if norms else ())
        return out if len(out) > 1 else out[0]

    def bond_purities(self, mps_set: MpsSet, norms: bool = False):
        """Purity tr(rho^2) of the reduced state left of every bond, for every state of an fp64 set: float64 of shape (n_states,
        n_sites - 1), column k - 1 the bond between qubits k - 1 and k (S_2 = -log purity); with ``norms=True`` also <psi|psi> (the
        bits of ``local_paulis``), as ``(purities, norms)``.  A one-site chain has a zero-length bond axis.  Synchronous."""
        info = mps_set.info()
        ns, n = info["n_states"], info["n_sites"]
        out = np.zeros((ns, max(n - 1, 1)), dtype=np.float64)  # (one spare element for a one-site chain: the pointer stays valid)
        nrm = np.zeros(ns, dtype=np.float64)
        _check(lib().qk_bond_purities_host(self._h, mps_set.handle, out.ctypes.data, nrm.ctypes.data), "qk_bond_purities_host")
        out = out[:, : n - 1]
        return (out, nrm) if norms else out

    def block_values_host(self, xset: MpsSet, yset: MpsSet | None, plan: Plan, widths, side="left") -> np.ndarray:
        """Reduced-state overlaps O_w = tr(rho_A(x_i) rho_A(y_j)) of ``plan``'s pairs, A = the first (``side="left"``) or last
        (``"right"``) w qubits, for every w of ``widths`` (strictly increasing, 1 .. n_sites): float64 of shape (n_widths,
        plan.num_pairs), pairs as ``plan.pairs()`` lists them.  One pair chain gives every width at once; a (pair, width) value is
        the same bits whatever the other pairs and widths of the call.  fp64 sets only.  Synchronous."""
        n = xset.info()["n_sites"]
        w = _block_widths(widths, n)
        vals = np.zeros((max(w.size, 1), max(plan.num_pairs, 1)), dtype=np.float64)  # (spare elements: the pointers stay valid)
        wp = w if w.size else np.zeros(1, dtype=np.int32)
        _check(lib().qk_block_values_host(self._h, xset.handle, None if yset is None else yset.handle, plan.handle, _block_side(side), int(w.size), wp.ctypes.data,
                                          vals.ctypes.data), "qk_block_values_host")
        return np.ascontiguousarray(vals[: w.size, : plan.num_pairs])

    def block_self(self, mps_set: MpsSet, widths=None, side="left", norms: bool = False):
        """Self overlaps S_w = tr(rho_A(psi)^2) -- the purity of the cut -- of every state of an fp64 set, through the route of
        ``block_values_host`` (the pairs (s, s)): float64 of shape (n_widths, n_states); ``widths=None`` means 1 .. n_sites.  With
        ``norms=True`` also <psi|psi> (the bits of ``local_paulis``), as ``(S, norms)``.  Synchronous."""
        info = mps_set.info()
        ns, n = info["n_states"], info["n_sites"]
        w = _block_widths(widths, n)
        out = np.zeros((max(w.size, 1), ns), dtype=np.float64)
        nrm = np.zeros(ns, dtype=np.float64)
        wp = w if w.size else np.zeros(1, dtype=np.int32)
        _check(lib().qk_block_self_host(self._h, mps_set.handle, _block_side(side), int(w.size), wp.ctypes.data, out.ctypes.data, nrm.ctypes.data), "qk_block_self_host")
        out = np.ascontiguousarray(out[: w.size])
        return (out, nrm) if norms else out

    def block_overlaps(self, xs: MpsSet, ys: MpsSet | None = None, widths=None, side="left"):
        """``(O, Sx, Sy)``: the reduced-state overlaps O[w, j, i] = tr(rho_A(x_i) rho_A(y_j)) of every pair, shape (n_widths, ny,
        nx), rows = Y (or X), and the self overlaps Sx (n_widths, nx), Sy (n_widths, ny) -- what ``block_kernel`` takes.
        ``widths=None`` means 1 .. n_sites.  A symmetric call (``ys=None``) computes the pairs i <= j, mirrors them, takes Sx from
        the diagonal (the bits of ``block_self``) and returns ``Sy = Sx``.  Synchronous."""
        sym = ys is None
        nx = len(xs)
        ny = nx if sym else len(ys)
        plan = Plan(xs.dims, None if sym else ys.dims, orient=False)
        try:
            vals = self.block_values_host(xs, ys, plan, widths, side)
            pairs = plan.pairs()
        finally:
            plan.close()
        O = np.zeros((vals.shape[0], ny, nx), dtype=np.float64)
        O[:, pairs[:, 1], pairs[:, 0]] = vals
        if sym:
            O[:, pairs[:, 0], pairs[:, 1]] = vals
            d = np.arange(nx)
            Sx = np.ascontiguousarray(O[:, d, d])
            return O, Sx, Sx
        return O, self.block_self(xs, widths, side), self.block_self(ys, widths, side)

    def shot_block_sums_host(self, bits_x, bits_y, settings, pairs, widths, side="left", per_setting: bool = False):
        """``engine.shot_block_sums`` on the device (``qk_shot_block_sums_host``): the same int64 sums, bit for bit, for outcome tables
        ``bits_x`` (nx, U M, n) and ``bits_y`` (ny, U M, n; ``None``: Y is X) of U = ``settings`` settings, the pairs (x index, y
        index) of ``pairs`` in any order and the strictly increasing ``widths`` in 1 .. min(n, 32) (``None``: all of them).  Returns
        ``sums`` (n_widths, n_pairs), with ``per_setting=True`` also S (n_widths, n_pairs, U).  It needs no MPS set.  Synchronous."""
        bx = np.ascontiguousarray(_shot_bits(bits_x, "bits_x"), dtype=np.uint8)
        by = None if bits_y is None else np.ascontiguousarray(_shot_bits(bits_y, "bits_y"), dtype=np.uint8)
        if by is not None and by.shape[1:] != bx.shape[1:]:
            raise ValueError(f"bits_x and bits_y differ in shots or qubits: {bx.shape} and {by.shape}")
        nx, shots, n = bx.shape
        U, M = _shot_split(shots, settings)
        w = _block_widths(widths, min(n, SHOT_BLOCK_MAX_WIDTH))
        P = np.ascontiguousarray(np.asarray(pairs).reshape(-1, 2), dtype=np.int32)
        sums = np.zeros((max(w.size, 1), max(len(P), 1)), dtype=np.int64)  # (spare elements: the pointers stay valid)
        S = np.zeros(sums.shape + (U,), dtype=np.int64) if per_setting else None
        wp = w if w.size else np.zeros(1, dtype=np.int32)
        pp = P if len(P) else np.zeros((1, 2), dtype=np.int32)
        _check(lib().qk_shot_block_sums_host(self._h, n, U, M, nx, bx.ctypes.data, nx if by is None else by.shape[0], None if by is None else by.ctypes.data, len(P),
                                             pp.ctypes.data, _block_side(side), int(w.size), wp.ctypes.data, sums.ctypes.data, None if S is None else S.ctypes.data),
               "qk_shot_block_sums_host")
        sums = np.ascontiguousarray(sums[: w.size, : len(P)])
        return (sums, np.ascontiguousarray(S[: w.size, : len(P)])) if per_setting else sums

    def shot_block_overlaps(self, bits_x, bits_y=None, settings=1, widths=None, side="left", stderr: bool = False):
        """``(O_hat, Sx_hat, Sy_hat)``: ``block_overlaps`` estimated from measurement shots by the randomised-measurement protocol --
        O_hat[w, j, i] estimates tr(rho_A(x_i) rho_A(y_j)), shape (n_widths, ny, nx), Sx_hat (n_widths, nx) and Sy_hat (n_widths, ny) the
        purities, what ``block_kernel`` takes.  ``bits_x`` (nx, U M, n) and ``bits_y`` are the bits ``Context.sample`` drew in
        ``setting_bases(U, M, n)`` with U = ``settings`` (every state in the same table); ``widths=None`` means 1 .. min(n, 32).  The
        estimate is unbiased for every width; its error is set by the spread from setting to setting, so spend shots on settings.
        A symmetric call (``bits_y=None``) computes the pairs i <= j and mirrors them; its diagonal is the purity estimate (the a == b
        shot pairs removed, M >= 2), the same bits as Sx_hat, and ``Sy_hat = Sx_hat``.  ``stderr=True`` also returns the standard
        errors ``(eO, eSx, eSy)`` in the same shapes (nan when U < 2).  Synchronous."""
        bx = _shot_bits(bits_x, "bits_x")
        nx = bx.shape[0]
        U, M = _shot_split(bx.shape[1], settings)

        def self_of(b):
            d = np.arange(b.shape[0])
            out = self.shot_block_sums_host(b, None, U, np.stack([d, d], axis=1), widths, side, per_setting=stderr)
            return shot_block_estimate(out[0] if stderr else out, out[1] if stderr else None, U, M, True)

        if bits_y is None:
            iu = np.triu_indices(nx)
            pairs = np.stack([iu[0], iu[1]], axis=1)  # i <= j
            out = self.shot_block_sums_host(bx, None, U, pairs, widths, side, per_setting=stderr)
            vals, errs = shot_block_estimate(out[0] if stderr else out, out[1] if stderr else None, U, M, pairs[:, 0] == pairs[:, 1])
            O, E = np.zeros((vals.shape[0], nx, nx)), np.zeros((vals.shape[0], nx, nx))
            for dst, src in ((O, vals), (E, errs)):
                dst[:, pairs[:, 1], pairs[:, 0]] = src
                dst[:, pairs[:, 0], pairs[:, 1]] = src
            d = np.arange(nx)
            Sx, Ex = np.ascontiguousarray(O[:, d, d]), np.ascontiguousarray(E[:, d, d])
            return ((O, Sx, Sx), (E, Ex, Ex)) if stderr else (O, Sx, Sx)
        by = _shot_bits(bits_y, "bits_y")
        ny = by.shape[0]
        jj, ii = np.divmod(np.arange(ny * nx), nx)
        out = self.shot_block_sums_host(bx, by, U, np.stack([ii, jj], axis=1), widths, side, per_setting=stderr)
        vals, errs = shot_block_estimate(out[0] if stderr else out, out[1] if stderr else None, U, M, False)
        O, E = vals.reshape(-1, ny, nx), errs.reshape(-1, ny, nx)
        (Sx, Ex), (Sy, Ey) = self_of(bx), self_of(by)
        return ((O, Sx, Sy), (E, Ex, Ey)) if stderr else (O, Sx, Sy)

    def shadow_hist_host(self, bits_x, bases_x, bits_y=None, bases_y=None, pairs=(), equal: bool = False):
        """``engine.shadow_hist`` on the device (``qk_shadow_hist_host``): the same int64 histograms, bit for bit.  ``bits_x``
        (nx, T_x, n) with ``bases_x`` (T_x, n) shared or (nx, T_x, n) per state, ``bits_y``/``bases_y`` likewise (both ``None``: Y is
        X), the pairs (x index, y index) of ``pairs`` in any order; n <= 128.  Returns H (n_pairs, 2 n + 1), with ``equal=True`` also
        the histogram of the pairs t = t' (T_x == T_y).  It needs no MPS set.  Synchronous."""
        bx, cx, xps = _shadow_tables(bits_x, bases_x, "x")
        bx, cx = np.ascontiguousarray(bx, dtype=np.uint8), np.ascontiguousarray(cx, dtype=np.uint8)
        by = cy = None
        yps = 0
        if bits_y is not None:
            if bases_y is None:
                raise ValueError("bits_y is given but bases_y is None")
            by, cy, yps = _shadow_tables(bits_y, bases_y, "y")
            by, cy = np.ascontiguousarray(by, dtype=np.uint8), np.ascontiguousarray(cy, dtype=np.uint8)
            if by.shape[2] != bx.shape[2]:
                raise ValueError(f"bits_x and bits_y differ in qubits: {bx.shape} and {by.shape}")
        elif bases_y is not None:
            cy = np.ascontiguousarray(np.asarray(bases_y), dtype=np.uint8)  # (rejected by the entry point: Y is X)
        nx, tx, n = bx.shape
        ny, ty = (nx, tx) if by is None else by.shape[:2]
        P = np.ascontiguousarray(np.asarray(pairs).reshape(-1, 2), dtype=np.int32)
        H = np.zeros((max(len(P), 1), 2 * n + 1), dtype=np.int64)  # (a spare row: the pointers stay valid)
        E = np.zeros_like(H) if equal else None
        pp = P if len(P) else np.zeros((1, 2), dtype=np.int32)
        _check(lib().qk_shadow_hist_host(self._h, n, nx, tx, bx.ctypes.data, cx.ctypes.data, xps, ny, ty, None if by is None else by.ctypes.data,
                                         None if cy is None else cy.ctypes.data, yps, len(P), pp.ctypes.data, H.ctypes.data, None if E is None else E.ctypes.data),
               "qk_shadow_hist_host")
        H = np.ascontiguousarray(H[: len(P)])
        return (H, np.ascontiguousarray(E[: len(P)])) if equal else H

    def shadow_hists(self, bits_x, bases_x, bits_y=None, bases_y=None, equal: bool = False):
        """The shot-pair histograms of every pair of two outcome tables, int64 of shape (ny, nx, 2 n + 1), what ``shadow_inner`` and
        ``shadow_kernel`` take: ``H[j, i]`` is the histogram of (x_i, y_j).  A symmetric call (``bits_y=None``) computes the pairs
        i <= j and mirrors them -- d is symmetric in its two shots -- and its diagonal holds the self pairs.  ``equal=True`` returns
        ``(H, E)`` with E the histograms of the pairs t = t' in the same shape.  Synchronous."""
        nx, n = _shot_bits(bits_x, "bits_x").shape[0], np.asarray(bits_x).shape[2]
        if bits_y is None:
            iu = np.triu_indices(nx)
            pairs = np.stack([iu[0], iu[1]], axis=1)  # i <= j
            out = self.shadow_hist_host(bits_x, bases_x, None, bases_y, pairs, equal)
            res = []
            for src in out if equal else (out,):
                dst = np.zeros((nx, nx, 2 * n + 1), dtype=np.int64)
                dst[pairs[:, 1], pairs[:, 0]] = src
                dst[pairs[:, 0], pairs[:, 1]] = src
                res.append(dst)
            return tuple(res) if equal else res[0]
        ny = _shot_bits(bits_y, "bits_y").shape[0]
        jj, ii = np.divmod(np.arange(ny * nx), nx)
        out = self.shadow_hist_host(bits_x, bases_x, bits_y, bases_y, np.stack([ii, jj], axis=1), equal)
        return tuple(o.reshape(ny, nx, 2 * n + 1) for o in out) if equal else out.reshape(ny, nx, 2 * n + 1)

    def shot_string_sums_host(self, bits, bases, strings):
        """``engine.shot_string_sums`` on the device (``qk_shot_strings_host``): the same int64 ``(sums, counts)``, bit for bit, both
        (n_states, m).  ``bits`` (n_states, shots, n) with ``bases`` (shots, n) shared or (n_states, shots, n) per state; ``strings``
        anything ``pauli_strings(n, ...)`` takes, or a code table (m, n); n <= 128.  It needs no MPS set.  Synchronous."""
        b, c, per_state = _string_tables(bits, bases)
        b, c = np.ascontiguousarray(b, dtype=np.uint8), np.ascontiguousarray(c, dtype=np.uint8)
        ns, T, n = b.shape
        S = _string_table(n, strings, checked=False)  # (the library rejects a code above 3 by the string's index)
        sums, counts = np.zeros((ns, S.shape[0]), dtype=np.int64), np.zeros((ns, S.shape[0]), dtype=np.int64)
        _check(lib().qk_shot_strings_host(self._h, n, ns, T, b.ctypes.data, c.ctypes.data, per_state, S.shape[0], S.ctypes.data, sums.ctypes.data, counts.ctypes.data),
               "qk_shot_strings_host")
        return sums, counts

    def estimate_pauli_strings(self, bits, bases, strings):
        """Expectation values of Pauli strings estimated from measurement shots, the finite-shot counterpart of
        ``pauli_expectations``: ``(values, counts)``, float64 and int64 of shape (n_states, m).  ``values[s, j]`` is the mean sign of
        the shots of state s whose bases equal string j on its support (``string_values`` of ``shot_string_sums_host``: 0.0 where no
        shot matches), ``counts[s, j]`` the number of those shots.  Arguments as ``shot_string_sums_host``.  Synchronous."""
        sums, counts = self.shot_string_sums_host(bits, bases, strings)
        return string_values(sums, counts), counts

    def estimate_window_rdms(self, bits, bases, width: int, starts=None):
        """Reduced density matrices of contiguous windows of ``width`` qubits (1 .. min(n, 6)) estimated from measurement shots, the
        finite-shot counterpart of ``window_rdms``: ``(rho_hat, counts)``.  ``rho_hat`` is complex128 (n_states, n_windows, 2^w,
        2^w), ``paulis_rdm`` of the estimated coefficients of the 4^w strings of each window (``window_strings``, windows as
        ``starts`` of ``window_rdms``); ``counts`` is int64 (n_states, n_windows) + (4,) * w, the shots behind each coefficient.
        ``rho_hat`` is exactly Hermitian with trace exactly 1 (the identity coefficient is exactly 1.0), but it is a linear
        inversion: it is NOT positive semi-definite in general -- at few shots it has negative eigenvalues of the order of the
        statistical error.  The projected kernels need only Frobenius distances, which stay meaningful.  Synchronous."""
        return estimate_window_rdms(bits, bases, width, starts, self.shot_string_sums_host)

    def bond_spectra(self, mps_set: MpsSet, max_values: int | None = None, norms: bool = False):
        """Entanglement spectra of every state of an fp64 set: the Schmidt weights (eigenvalues of the reduced state, descending, sum
        1) across every bond, float64 of shape (n_states, n_sites - 1, m), zero beyond a bond's true dimension.  ``max_values=m``
        keeps the m largest weights of each bond; the default is the set's largest true bond (every weight).  ``norms=True``
        adds <psi|psi> (the bits of ``local_paulis``).  ``bond_entropies``, ``cap_cost`` and ``schmidt_rank`` read the result.
        Weights below about 1e-15 are rounding noise.  Synchronous."""
        info = mps_set.info()
        ns, n = info["n_states"], info["n_sites"]
        if max_values is None:
            m = int(np.asarray(mps_set.dims)[:, 1:n].max()) if n > 1 else 1
        else:
            if isinstance(max_values, bool) or not isinstance(max_values, (int, np.integer)):
                raise ValueError(f"max_values must be an int >= 1 or None (every weight), got {max_values!r}")
            m = int(max_values)
        out = np.zeros((ns, max(n - 1, 1), max(m, 1)), dtype=np.float64)
        nrm = np.zeros(ns, dtype=np.float64)
        _check(lib().qk_bond_spectra_host(self._h, mps_set.handle, m, out.ctypes.data, nrm.ctypes.data), "qk_bond_spectra_host")
        out = out[:, : n - 1]
        return (out, nrm) if norms else out

    def compress(self, mps_set: MpsSet, max_bond: int | None = None, max_discard: float = 0.0, value_of_zero: float = 1e-16, info: bool = False):
        """A new fp64 set with every state of ``mps_set`` truncated once, in canonical form (the device twin of ``MPS.compress``,
        which documents the rule): at most ``max_bond`` values per bond (``None`` or 0: no cap), at most ``max_discard`` of the weight
        dropped per bond, singular values <= ``value_of_zero`` sqrt(weight) dropped.  Norms are kept, sites 0 .. n-2 of the result
        are left isometries, its ``.dims`` is the new bond table; ``mps_set`` is left untouched.  ``info=True`` returns ``(set,
        {"fidelity": (n_states,), "discarded": (n_states, n_sites - 1), "bond_dims": (n_states, n_sites + 1)})`` with fidelity =
        |<psi|psi'>|^2 / (<psi|psi> <psi'|psi'>), the product over the bonds of 1 - discarded.  A state's result is the same bits
        whatever the other states of the set.  Synchronous."""
        cap = 0 if max_bond is None else max_bond
        if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)):
            raise ValueError(f"max_bond must be an int >= 0 or None (no cap), got {max_bond!r}")
        st = mps_set.info()
        ns, n = st["n_states"], st["n_sites"]
        fid = np.zeros(ns, dtype=np.float64)
        disc = np.zeros((ns, max(n - 1, 1)), dtype=np.float64)
        h = _P()
        _check(lib().qk_mps_set_compress(self._h, mps_set.handle, int(cap), float(max_discard), float(value_of_zero), C.byref(h), fid.ctypes.data, disc.ctypes.data),
               "qk_mps_set_compress")
        out = MpsSet(self, h, np.zeros((ns, n + 1), dtype=np.int32))
        out.dims = out.image()[2]
        if not info:
            return out
        return out, {"fidelity": fid, "discarded": disc[:, : n - 1], "bond_dims": out.dims.copy()}

    def window_rdms(self, xs: MpsSet, width: int, starts=None, norms: bool = False):
        """Reduced density matrices of contiguous windows of ``width`` qubits (1 .. min(n_sites, 6)) of every state of an fp64
        set: complex128 of shape (n_states, n_windows, 2^w, 2^w), window i = the qubits starts[i] .. starts[i] + width - 1, row index
        s = sum_j s_{start+j} 2^(w-1-j).  ``starts=None`` means every window 0 .. n_sites - width; otherwise strictly increasing
        ints in that range.  rho is exactly Hermitian, tr rho = 1 to rounding, and a (state, window) value is the same bits
        whatever the other states and windows of the call.  With ``norms=True`` also <psi|psi> (the bits of ``local_paulis``), as
        ``(rho, norms)``.  Synchronous."""
        info = xs.info()
        ns, n = info["n_states"], info["n_sites"]
        if isinstance(width, bool) or not isinstance(width, (int, np.integer)):
            raise ValueError(f"width must be an int, got {width!r}")
        w = int(width)
        st = None
        if starts is not None:
            st = np.asarray(starts)
            if st.ndim != 1 or (st.size and not np.issubdtype(st.dtype, np.integer)) or st.dtype == np.bool_:
                raise ValueError(f"starts must be a list of ints, got {starts!r}")
            st = np.ascontiguousarray(st, dtype=np.int32)
        ok = 1 <= w <= min(n, WINDOW_MAX_WIDTH)  # (the library rejects a bad width or start: spare elements keep the pointers valid)
        nw = (n - w + 1 if ok else 1) if st is None else max(int(st.size), 1)
        D = 1 << (w if ok else 1)
        rho = np.zeros((ns, nw, D, D), dtype=np.complex128)
        nrm = np.zeros(ns, dtype=np.float64)
        sp = None if st is None else (st if st.size else np.zeros(1, dtype=np.int32))
        _check(lib().qk_window_rdms_host(self._h, xs.handle, w, 0 if st is None else int(st.size), None if sp is None else sp.ctypes.data, rho.ctypes.data,
                                         nrm.ctypes.data), "qk_window_rdms_host")
        return (rho, nrm) if norms else rho

    def projected_window_gram(self, rx, ry=None, gamma=None) -> np.ndarray:
        """The k-qubit projected quantum kernel K[j, i] = exp(-gamma sum_a ||rho_a(x_i) - rho_a(y_j)||_F^2) of window RDMs
        (``window_rdms``): shape (ny, nx), rows = Y (or X) -- ``feature_gram`` at gamma over the columns (Re rho, Im rho).
        ``gamma=None`` means 1 / (n_windows + width - 1), which is 1 / n_sites when every window was taken.  Synchronous."""
        x, w = _window_rdms(rx, "rx")
        g = projected_gamma(gamma, x.shape[1] + w - 1)
        fy = None
        if ry is not None:
            y, wy = _window_rdms(ry, "ry")
            if wy != w or y.shape[1] != x.shape[1]:
                raise ValueError(f"Y RDMs of shape {y.shape} do not match X RDMs of shape {x.shape}")
            fy = window_columns(y)
        return self.feature_gram(window_columns(x), fy, g)

    def feature_gram(self, fx, fy=None, gamma=None) -> np.ndarray:
        """Gram of real feature columns (``pauli_expectations``): K[j, i] = exp(-gamma sum_m (fx[i, m] - fy[j, m])^2), shape (ny, nx),
        rows = Y (or X).  ``gamma=None`` means 1 / n_features.  Synchronous."""
        fx = np.ascontiguousarray(fx, dtype=np.float64)
        if fx.ndim != 2 or fx.shape[1] < 1:
            raise ValueError(f"features must have shape (n_states, n_features) with n_features >= 1, got {fx.shape}")
        nx, m = fx.shape
        g = projected_gamma(gamma, m)
        if fy is not None:
            fy = np.ascontiguousarray(fy, dtype=np.float64)
            if fy.ndim != 2 or fy.shape[1] != m:
                raise ValueError(f"Y features of shape {fy.shape} do not match X features of shape {fx.shape}")
        ny = nx if fy is None else fy.shape[0]
        out = np.zeros((ny, nx), dtype=np.float64)
        _check(lib().qk_feature_gram_host(self._h, m, nx, fx.ctypes.data, ny, None if fy is None else fy.ctypes.data, g, out.ctypes.data, nx),
               "qk_feature_gram_host")
        return out

    def stats(self) -> dict:
        st = QkStats()
        _check(lib().qk_get_stats(self._h, C.byref(st)), "qk_get_stats")
        d = st.as_dict()
        d["kernel_name"] = lib().qk_kernel_name(st.kernel, st.precision).decode()
        d["second_kernel_name"] = lib().qk_kernel_name(st.second_kernel, st.precision).decode() if st.second_kernel else ""
        return d

    def close(self):
        if self._h:
            self._close_sets()
            if not getattr(self, "_borrowed", False):  # a communicator's contexts die with the communicator
                lib().qk_ctx_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Comm:
    """The multi-GPU part of the C ABI (``qk_comm_*``): ONE process drives k MI355X of a node; RCCL over xGMI is reached
    inside the library (``ncclCommInitAll`` / ``ncclAllGather``), not through torch.  What the reference does with an
    mpi4py communicator and one process per GPU (/root/reference/gpu_backend/kernel_state_ansatz.py:149-199, 415-428)."""

    def __init__(self, n_devices: int | None = None, device_ids=None):
        if device_ids is not None:
            ids = np.ascontiguousarray(device_ids, dtype=np.int32)
            n_devices = int(ids.shape[0])
        else:
            ids = None
            n_devices = int(n_devices or device_count())
        h = _P()
        _check(lib().qk_comm_init_all(n_devices, None if ids is None else ids.ctypes.data, C.byref(h)), "qk_comm_init_all")
        self._h, self.size = h, int(lib().qk_comm_size(h))
        self._ctx = []
        for r in range(self.size):
            c = Context.__new__(Context)
            c._h, c.device_id, c._borrowed = _P(lib().qk_comm_ctx(h, r)), int(ids[r]) if ids is not None else r, True
            self._ctx.append(c)

    def ctx(self, rank: int) -> "Context":
        return self._ctx[rank]

    def allgather_sets(self, local, lo, total: int):
        """``local[r]``: the MpsSet of the states ``[lo[r], lo[r] + len(local[r]))`` on rank r's context (``None`` = empty
        share).  ONE all-gather of the packed images; returns the whole set on every device."""
        hs = (_P * self.size)(*[(m.handle if m is not None else None) for m in local])
        lo_a = np.ascontiguousarray(lo, dtype=np.int32)
        out = (_P * self.size)()
        _check(lib().qk_mps_set_allgather(self._h, hs, lo_a.ctypes.data, int(total), out), "qk_mps_set_allgather")
        n_sites = next(m for m in local if m is not None).dims.shape[1] - 1
        dims = np.zeros((total, n_sites + 1), dtype=np.int32)
        for m, l0 in zip(local, lo):
            if m is not None:
                dims[l0 : l0 + len(m)] = m.dims
        return [MpsSet(self._ctx[r], _P(out[r]), dims.copy()) for r in range(self.size)]

    def gram(self, xsets, ysets=None) -> np.ndarray:
        """The sharded Gram: one sweep launch per device, ONE all-gather of the packed values, a scatter per device;
        returns rank 0's dense matrix (rows = Y, cols = X)."""
        nx = len(xsets[0])
        ny = nx if ysets is None else len(ysets[0])
        xs = (_P * self.size)(*[m.handle for m in xsets])
        ys = None if ysets is None else (_P * self.size)(*[m.handle for m in ysets])
        out = np.zeros((ny, nx), dtype=np.float64)
        _check(lib().qk_gram_sharded(self._h, xs, ys, out.ctypes.data, nx), "qk_gram_sharded")
        return out

    def device_gram_ptr(self, rank: int) -> int:
        p = _P()
        _check(lib().qk_comm_device_gram(self._h, rank, C.byref(p)), "qk_comm_device_gram")
        return int(p.value or 0)

    def stats(self, rank: int = 0):
        st, ms = QkStats(), C.c_double()
        _check(lib().qk_comm_stats(self._h, rank, C.byref(st), C.byref(ms)), "qk_comm_stats")
        d = st.as_dict()
        d["kernel_name"] = lib().qk_kernel_name(st.kernel, st.precision).decode()
        d["allgather_ms"] = ms.value
        return d

    def close(self):
        if self._h:
            for c in self._ctx:  # sets made on the communicator's contexts (uploads, all-gathered sets) go first: their handles point
                c._close_sets()  # into contexts that qk_comm_destroy deletes
                c._h = None
            lib().qk_comm_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


_default_ctx: dict[int, Context] = {}


def default_context(device_id: int = 0) -> Context:
    if device_id not in _default_ctx:
        _default_ctx[device_id] = Context(device_id)
    return _default_ctx[device_id]


@contextmanager
def context(device_id: int = 0):
    ctx = Context(device_id)
    try:
        yield ctx
    finally:
        ctx.close()
