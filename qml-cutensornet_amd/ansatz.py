"""Feature-map ansatz as a compiled gate *program* (no pytket, no sympy).

Host-side mirror of the reference's ``KernelStateAnsatz``
(/root/reference/gpu_backend/kernel_state_ansatz.py:16-103).  The reference keeps
a symbolic pytket circuit and substitutes sympy symbols per data point; here the
circuit is compiled once into flat integer/float arrays and binding a data point
is one vectorised numpy expression.  The gate semantics are those of the
reference:

* H on every qubit when ``hadamard_init``                      (ref :53-55)
* per layer: Rz with half-turn exponent (2/pi)*gamma*f_i       (ref :58-60)
*            XXPhase with exponent gamma^2 (1-f_a)(1-f_b)      (ref :62-66)
* a non-adjacent XXPhase is routed eagerly: SWAP chain up, the gate on the last
  adjacent pair, SWAP chain down                               (ref :68-88)

Angles are pytket half-turns (theta = pi*alpha/2), the convention spelled out in
/root/reference/KernelPkg/src/KernelPkg.jl:8-32.

Custom feature maps (``CircuitAnsatz``, ``BoundCircuit.from_gates``) add Rx, Ry,
YYPhase and ZZPhase (op codes 4-7) to the four gates above; the matrices are
TKET's, as in KernelPkg.jl and the reference's CPU gate list.

Matrix gates (op codes 8 and 9) close the vocabulary: a 2x2 unitary on one qubit
(``Unitary1q``) and a 4x4 unitary on an adjacent pair (``Unitary2q``), read from a
table ``mats`` (complex128 [n_mats][4][4]; a 2x2 sits in ``[:2, :2]``) through a
per-gate index ``mat``.  The 4x4 index is (s_q, s_{q+1}) with qubit q most
significant (TKET's order).  The named constants X, Y, Z, S, Sdg, T, Tdg, V, Vdg,
SX, SXdg, CX, CY, CZ are entries of that table.

Op code 10 (``Kraus1q``) is a one-qubit Kraus channel applied at the orthogonality
centre: channel c is 1 <= m_c <= 4 complex 2x2 matrices ``kraus[c][:m_c]`` (table
complex128 [n_channels][4][2][2] plus ``n_kraus``), gate i reads channel
``channel[i]`` and either draws its branch as a quantum trajectory (``branch[i]`` =
-1) or takes the forced branch ``branch[i]`` (projectors, post-selection, replay).
Project, Measure, PostSelect, AmplitudeDamping, PhaseDamping, Depolarizing, BitFlip
and PhaseFlip are entries of that table.

Op code 11 (``Kraus2q``) is a two-qubit Kraus channel on the pair (q0, q0+1): channel
c is 1 <= m_c <= 16 complex 4x4 matrices ``kraus2[c][:m_c]`` (table complex128
[n_channels2][16][4][4] plus ``n_kraus2``; the index convention of ``Unitary2q``),
applied to theta = A_q A_{q+1} in front of the SVD of a two-qubit gate.  ``channel``
and ``branch`` are shared with code 10: where ``op`` is 11, ``channel[i]`` indexes
``kraus2``.  Project2q, Depolarizing2q, CorrelatedPhaseFlip, Measure2q and
PostSelect2q are entries of that table.

Classical control: two optional rows ride with a program that has a channel table.
``cond_gate[i]`` is -1 (gate i is unconditional) or the position g < i of a gate of op
code 10 or 11; ``cond_mask[i]`` (uint32) has bit v set when branch v of gate g lets
gate i run.  With b the branch recorded for gate g, gate i runs when b >= 0 and bit b of
the mask is set; else it is skipped: it does nothing at all (no centre move, no SVD, no
draw, no change of ``logw``), and a skipped channel gate records branch -2.  In gate
lists a fourth element ``(g, values)`` names the list position of an earlier channel
gate and the branches that let the gate run.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

OP_H, OP_RZ, OP_XX, OP_SWAP = 0, 1, 2, 3
OP_RX, OP_RY, OP_YY, OP_ZZ = 4, 5, 6, 7  # custom feature maps (CircuitAnsatz, BoundCircuit.from_gates)
OP_M1, OP_M2 = 8, 9  # matrix gates: a 2x2 on q0, a 4x4 on (q0, q0+1); the matrix of gate i is mats[mat[i]]
N_OPS = 8  # codes 0 .. N_OPS-1 are valid without a matrix table; every builder rejects any other
N_OPS_MAT = 10  # codes 0 .. N_OPS_MAT-1 are valid in a program that comes with a matrix table
OP_K1 = 10  # a one-qubit Kraus channel on q0, drawn or forced: valid only in a program that comes with a channel table
OP_K2 = 11  # a two-qubit Kraus channel on (q0, q0+1), drawn or forced: valid only in a program that comes with a two-qubit channel table
MAX_KRAUS = 4  # matrices per channel
MAX_KRAUS2 = 16  # matrices per two-qubit channel
TRACE_TOL = 1e-12  # max |sum_k K_k^H K_k - 1| a drawn channel may have
UNITARY_TOL = 1e-12  # max |M^H M - 1| a matrix gate may have: the builders' canonical-form bookkeeping assumes unitary gates
_OP_NAMES = {OP_H: "H", OP_RZ: "Rz", OP_XX: "XXPhase", OP_SWAP: "SWAP", OP_RX: "Rx", OP_RY: "Ry", OP_YY: "YYPhase", OP_ZZ: "ZZPhase",
             OP_M1: "Unitary1q", OP_M2: "Unitary2q", OP_K1: "Kraus1q", OP_K2: "Kraus2q"}
_OP_CODES = {name: code for code, name in _OP_NAMES.items()}
_TWO_QUBIT = (OP_XX, OP_SWAP, OP_YY, OP_ZZ, OP_M2, OP_K2)
_CHANNEL = (OP_K1, OP_K2)
_PARAMETRISED = (OP_RZ, OP_XX, OP_RX, OP_RY, OP_YY, OP_ZZ)
_MATRIX = (OP_M1, OP_M2)

_R2 = 0.7071067811865476
_NAMED_1Q = {  # TKET's matrices
    "X": [[0, 1], [1, 0]], "Y": [[0, -1j], [1j, 0]], "Z": [[1, 0], [0, -1]],
    "S": [[1, 0], [0, 1j]], "Sdg": [[1, 0], [0, -1j]],
    "T": [[1, 0], [0, complex(_R2, _R2)]], "Tdg": [[1, 0], [0, complex(_R2, -_R2)]],
    "V": [[_R2, -1j * _R2], [-1j * _R2, _R2]], "Vdg": [[_R2, 1j * _R2], [1j * _R2, _R2]],
    "SX": [[0.5 + 0.5j, 0.5 - 0.5j], [0.5 - 0.5j, 0.5 + 0.5j]], "SXdg": [[0.5 - 0.5j, 0.5 + 0.5j], [0.5 + 0.5j, 0.5 - 0.5j]],
}
_NAMED_2Q = {  # control first: index (s_control, s_target)
    "CX": [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]],
    "CY": [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, -1j], [0, 0, 1j, 0]],
    "CZ": [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, -1]],
}
_NAMED = {**_NAMED_1Q, **_NAMED_2Q}
_CHANNEL_NAMES = ("Kraus1q", "Project", "Measure", "PostSelect", "AmplitudeDamping", "PhaseDamping", "Depolarizing", "BitFlip", "PhaseFlip")
_CHANNEL2_NAMES = ("Kraus2q", "Project2q", "Depolarizing2q", "CorrelatedPhaseFlip", "Measure2q", "PostSelect2q")


def channel_kraus(name, params, where="channel"):
    """The Kraus matrices and the forced branch of a named channel: ``(K complex128 [m, 2, 2], branch)`` with ``branch`` -1 for a
    channel that is drawn.  ``K[k][s'][s] = <s'|K_k|s>``.
      * ``Kraus1q  [[K0, ..]]``: 1 .. 4 matrices as given, drawn;
      * ``Project  [M]``: the one matrix M, forced (any finite 2x2: a projector, a weak measurement's operator);
      * ``Measure  []``: P0 = |0><0|, P1 = |1><1|, drawn;
      * ``PostSelect [bit]``: P0, P1 with the branch ``bit`` forced;
      * ``AmplitudeDamping [g]``: [[1, 0], [0, sqrt(1-g)]], [[0, sqrt g], [0, 0]];
      * ``PhaseDamping [lam]``: [[1, 0], [0, sqrt(1-lam)]], [[0, 0], [0, sqrt lam]];
      * ``Depolarizing [p]``: sqrt(1 - 3p/4) I, sqrt(p/4) X, sqrt(p/4) Y, sqrt(p/4) Z;
      * ``BitFlip [p]``: sqrt(1-p) I, sqrt p X;   ``PhaseFlip [p]``: sqrt(1-p) I, sqrt p Z.
    ``ValueError`` for a wrong parameter count, a probability outside [0, 1] or matrices of the wrong shape."""
    if name not in _CHANNEL_NAMES:
        raise ValueError(f"unknown channel {name!r} (supported: {', '.join(_CHANNEL_NAMES)})")
    I2, X, Y, Z = np.eye(2), np.array(_NAMED_1Q["X"]), np.array(_NAMED_1Q["Y"]), np.array(_NAMED_1Q["Z"])
    P0, P1 = np.diag([1.0, 0.0]), np.diag([0.0, 1.0])
    if name in ("Kraus1q", "Project"):
        try:
            K = np.asarray(params, dtype=np.complex128)
        except (TypeError, ValueError):
            raise ValueError(f"{where} ({name}): the parameter must be a list of complex 2x2 matrices") from None
        if K.ndim == 4 and K.shape[0] == 1:
            K = K[0]
        if name == "Project":
            if K.shape == (2, 2):
                K = K[None]
            if K.shape != (1, 2, 2):
                raise ValueError(f"{where} (Project): expected one 2x2 matrix, got shape {K.shape}")
            return np.ascontiguousarray(K), 0
        if K.ndim != 3 or K.shape[1:] != (2, 2) or not 1 <= K.shape[0] <= MAX_KRAUS:
            raise ValueError(f"{where} (Kraus1q): expected a list of 1..{MAX_KRAUS} 2x2 matrices, got shape {K.shape}")
        return np.ascontiguousarray(K), -1
    params = [] if params is None else list(np.ravel(params))
    want = 0 if name == "Measure" else 1
    if len(params) != want:
        raise ValueError(f"{where} ({name}): expected {want} parameter(s), got {params}")
    if name == "Measure":
        return np.stack([P0, P1]).astype(np.complex128), -1
    if name == "PostSelect":
        if params[0] not in (0, 1):
            raise ValueError(f"{where} (PostSelect): the bit must be 0 or 1, got {params[0]!r}")
        return np.stack([P0, P1]).astype(np.complex128), int(params[0])
    p = float(params[0])
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"{where} ({name}): the parameter must lie in [0, 1], got {p!r}")
    if name == "AmplitudeDamping":
        K = [np.diag([1.0, np.sqrt(1.0 - p)]), np.array([[0.0, np.sqrt(p)], [0.0, 0.0]])]
    elif name == "PhaseDamping":
        K = [np.diag([1.0, np.sqrt(1.0 - p)]), np.diag([0.0, np.sqrt(p)])]
    elif name == "Depolarizing":
        K = [np.sqrt(1.0 - 0.75 * p) * I2, np.sqrt(0.25 * p) * X, np.sqrt(0.25 * p) * Y, np.sqrt(0.25 * p) * Z]
    elif name == "BitFlip":
        K = [np.sqrt(1.0 - p) * I2, np.sqrt(p) * X]
    else:
        K = [np.sqrt(1.0 - p) * I2, np.sqrt(p) * Z]
    return np.stack(K).astype(np.complex128), -1


def channel_kraus2(name, params, where="channel"):
    """The Kraus matrices and the forced branch of a named two-qubit channel on the pair [a, b]: ``(K complex128 [m, 4, 4], branch)``
    with ``branch`` -1 for a channel that is drawn.  ``K[k][(p,p')][(s,s')]``, qubit a most significant (the order of ``Unitary2q``).
      * ``Kraus2q  [[K0, ..]]``: 1 .. 16 matrices as given, drawn;
      * ``Project2q  [M]``: the one matrix M, forced (any finite 4x4);
      * ``Depolarizing2q [p]``: sqrt(1 - 15p/16) I(x)I and sqrt(p/16) P(x)Q for the 15 other Pauli pairs, P-major over I, X, Y, Z;
      * ``CorrelatedPhaseFlip [p]``: sqrt(1-p) I(x)I, sqrt p Z(x)Z;
      * ``Measure2q  []``: the four projectors |ss'><ss'|, drawn;
      * ``PostSelect2q [bits]``: the four projectors with the branch ``bits`` (0..3, qubit a most significant) forced.
    ``ValueError`` for a wrong parameter count, a probability outside [0, 1] or matrices of the wrong shape."""
    if name not in _CHANNEL2_NAMES:
        raise ValueError(f"unknown two-qubit channel {name!r} (supported: {', '.join(_CHANNEL2_NAMES)})")
    if name in ("Kraus2q", "Project2q"):
        try:
            K = np.asarray(params, dtype=np.complex128)
        except (TypeError, ValueError):
            raise ValueError(f"{where} ({name}): the parameter must be a list of complex 4x4 matrices") from None
        if K.ndim == 4 and K.shape[0] == 1:
            K = K[0]
        if name == "Project2q":
            if K.shape == (4, 4):
                K = K[None]
            if K.shape != (1, 4, 4):
                raise ValueError(f"{where} (Project2q): expected one 4x4 matrix, got shape {K.shape}")
            return np.ascontiguousarray(K), 0
        if K.ndim != 3 or K.shape[1:] != (4, 4) or not 1 <= K.shape[0] <= MAX_KRAUS2:
            raise ValueError(f"{where} (Kraus2q): expected a list of 1..{MAX_KRAUS2} 4x4 matrices, got shape {K.shape}")
        return np.ascontiguousarray(K), -1
    params = [] if params is None else list(np.ravel(params))
    want = 0 if name == "Measure2q" else 1
    if len(params) != want:
        raise ValueError(f"{where} ({name}): expected {want} parameter(s), got {params}")
    proj = np.zeros((4, 4, 4), dtype=np.complex128)
    proj[np.arange(4), np.arange(4), np.arange(4)] = 1.0
    if name == "Measure2q":
        return proj, -1
    if name == "PostSelect2q":
        if params[0] not in (0, 1, 2, 3):
            raise ValueError(f"{where} (PostSelect2q): the bits must be 0..3, got {params[0]!r}")
        return proj, int(params[0])
    p = float(params[0])
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"{where} ({name}): the parameter must lie in [0, 1], got {p!r}")
    pauli = [np.eye(2), np.array(_NAMED_1Q["X"]), np.array(_NAMED_1Q["Y"]), np.array(_NAMED_1Q["Z"])]
    if name == "Depolarizing2q":
        K = [np.sqrt(p / 16.0) * np.kron(P, Q) for P in pauli for Q in pauli]
        K[0] = np.sqrt(1.0 - 15.0 * p / 16.0) * np.eye(4)
    else:
        K = [np.sqrt(1.0 - p) * np.eye(4), np.sqrt(p) * np.kron(pauli[3], pauli[3])]
    return np.stack(K).astype(np.complex128), -1


class _ChannelTable:
    """The channel table of a program under construction: every channel gate takes a slot of its own, by structure.  ``d`` = 2: the
    one-qubit channels of op code 10; ``d`` = 4: the two-qubit channels of op code 11."""

    def __init__(self, d=2):
        self.entries, self.d = [], d

    def slot(self, name, params, where, exchange=False):
        """(slot, forced branch or -1) of one channel gate as given; ``exchange``: a two-qubit channel named on [a, b] with a > b,
        every matrix with the roles of its qubits exchanged (the rule of ``Unitary2q``)."""
        K, branch = channel_kraus(name, params, where) if self.d == 2 else channel_kraus2(name, params, where)
        if not np.all(np.isfinite(K)):
            raise ValueError(f"{where} ({name}): a Kraus matrix has an entry that is not finite")
        if branch < 0:
            dev = float(np.abs(np.einsum("kba,kbc->ac", K.conj(), K) - np.eye(self.d)).max())
            if not dev <= TRACE_TOL:
                raise ValueError(f"{where} ({name}): the channel is not trace preserving (max |sum K^H K - 1| = {dev:.3e} > {TRACE_TOL:g})")
        if exchange:
            K = np.stack([exchange_qubits(k) for k in K])
        self.entries.append(K)
        return len(self.entries) - 1, branch

    def arrays(self):
        kraus = np.zeros((len(self.entries), self.d * self.d, self.d, self.d), dtype=np.complex128)
        for c, K in enumerate(self.entries):
            kraus[c, : K.shape[0]] = K
        return kraus, np.asarray([K.shape[0] for K in self.entries], dtype=np.int32)


def is_two_qubit(o) -> bool:
    """Does op code ``o`` act on the pair (q0, q0+1)?  XXPhase, SWAP, YYPhase, ZZPhase, the 4x4 matrix gate and the two-qubit
    Kraus channel do."""
    return o in _TWO_QUBIT


def check_op_codes(op, with_table: bool = False, with_channels: bool = False, with_channels2: bool = False) -> None:
    """``ValueError`` unless every code of ``op`` is one of the N_OPS gates -- or, in a program that comes with a matrix table
    (``with_table``), one of the N_OPS_MAT; code 10 is valid in a program that comes with a channel table (``with_channels``), code
    11 in one that comes with a two-qubit channel table (``with_channels2``)."""
    op = np.asarray(op)
    top = N_OPS_MAT if with_table else N_OPS
    bad = (op < 0) | (op >= top)
    if with_channels:
        bad &= op != OP_K1
    if with_channels2:
        bad &= op != OP_K2
    if bad.any():
        raise ValueError(f"unknown gate op code {int(op[bad][0])} (valid: 0..{top - 1}{', 10' if with_channels else ''}{', 11' if with_channels2 else ''})")


def exchange_qubits(m4) -> np.ndarray:
    """A 4x4 with the roles of its two qubits exchanged: M'[(t,s)][(t',s')] = M[(s,t)][(s',t')]."""
    return np.ascontiguousarray(np.asarray(m4, dtype=np.complex128).reshape(2, 2, 2, 2).transpose(1, 0, 3, 2).reshape(4, 4))


def check_unitary(m, where) -> None:
    """``ValueError`` unless the square matrix ``m`` is finite and max |M^H M - 1| <= UNITARY_TOL; ``where`` names the gate."""
    if not np.all(np.isfinite(m)):
        raise ValueError(f"{where}: the matrix has an entry that is not finite")
    dev = float(np.abs(m.conj().T @ m - np.eye(m.shape[0])).max())
    if not dev <= UNITARY_TOL:
        raise ValueError(f"{where}: the matrix is not unitary (max |M^H M - 1| = {dev:.3e} > {UNITARY_TOL:g})")


def check_matrix_gates(op, mat, mats, with_channels: bool = False, with_channels2: bool = False):
    """The matrix table of a program, validated: ``(mat int32 [n_gates], mats complex128 [n_mats, 4, 4])``, or ``(None, None)``
    for a program without one (its codes 8 and 9 are then unknown: ``check_op_codes``).  ``ValueError`` when the table is not
    [n_mats][4][4], when ``mat`` of a matrix gate lies outside 0 .. n_mats-1, or when the 2x2 (``[:2, :2]`` of the slot) or 4x4
    the gate reads is not finite and unitary to UNITARY_TOL; the message names the gate's position in the program."""
    op = np.asarray(op)
    if mats is None or mat is None:
        check_op_codes(op, with_channels=with_channels, with_channels2=with_channels2)
        return None, None
    check_op_codes(op, with_table=True, with_channels=with_channels, with_channels2=with_channels2)
    mats = np.asarray(mats)
    if mats.ndim != 3 or mats.shape[1:] != (4, 4):
        raise ValueError(f"the matrix table must be [n_mats][4][4], got shape {mats.shape}")
    mats = np.ascontiguousarray(mats, dtype=np.complex128)
    mat = np.ascontiguousarray(mat, dtype=np.int32)
    if mat.shape != op.shape:
        raise ValueError(f"mat must hold one index per gate of the program ({op.shape[0]}), got shape {mat.shape}")
    seen = set()
    for i in np.flatnonzero((op == OP_M1) | (op == OP_M2)):
        k, d = int(mat[i]), 2 if op[i] == OP_M1 else 4
        if not 0 <= k < mats.shape[0]:
            raise ValueError(f"gate {int(i)}: matrix index {k} outside 0..{mats.shape[0] - 1}")
        if (k, d) not in seen:
            check_unitary(mats[k, :d, :d], f"gate {int(i)} ({_OP_NAMES[int(op[i])]}, table entry {k})")
            seen.add((k, d))
    return mat, mats


def check_channel_gates(op, q0, n_qubits, channel, branch, kraus, n_kraus, kraus2=None, n_kraus2=None):
    """The channel tables of a program, validated: ``(channel int32 [n_gates], branch int32 [n_gates], kraus complex128
    [n_channels, 4, 2, 2], n_kraus int32 [n_channels], kraus2 complex128 [n_channels2, 16, 4, 4], n_kraus2 int32 [n_channels2])``
    -- a table that is absent comes back as ``None, None``, its code (10 / 11) is then unknown --, or ``None`` for a program with
    neither.  ``ValueError``, naming the gate's position, when a channel gate's ``channel`` lies outside its table, its count of
    matrices outside 1 .. 4 (1 .. 16 for code 11), one of its matrices has an entry that is not finite, its ``branch`` lies outside
    -1 .. m-1, a drawn channel is not trace preserving (max |sum_k K_k^H K_k - 1| > TRACE_TOL; a forced branch may be any finite
    matrix) or the gate lies outside the register."""
    one = kraus is not None and n_kraus is not None
    two = kraus2 is not None and n_kraus2 is not None
    if channel is None or not (one or two):
        return None
    op = np.asarray(op)
    tables = {}
    for code, d, k, nk in ((OP_K1, 2, kraus, n_kraus), (OP_K2, 4, kraus2, n_kraus2)):
        if k is None or nk is None:
            tables[code] = (d, None, None)
            continue
        k = np.asarray(k)
        if k.ndim != 4 or k.shape[1:] != (d * d, d, d):
            raise ValueError(f"the {'two-qubit ' if d == 4 else ''}channel table must be [n_channels][{d * d}][{d}][{d}], got shape {k.shape}")
        k, nk = np.ascontiguousarray(k, dtype=np.complex128), np.ascontiguousarray(nk, dtype=np.int32)
        if nk.shape != k.shape[:1]:
            raise ValueError(f"n_kraus{'2' if d == 4 else ''} must hold one count per channel ({k.shape[0]}), got shape {nk.shape}")
        tables[code] = (d, k, nk)
    channel = np.ascontiguousarray(channel, dtype=np.int32)
    branch = np.full(op.shape, -1, dtype=np.int32) if branch is None else np.ascontiguousarray(branch, dtype=np.int32)
    if channel.shape != op.shape or branch.shape != op.shape:
        raise ValueError(f"channel and branch must hold one entry per gate ({op.shape[0]}); got shapes {channel.shape}, {branch.shape}")
    q0 = np.asarray(q0)
    for i in np.flatnonzero((op == OP_K1) | (op == OP_K2)):
        d, table, counts = tables[int(op[i])]
        if table is None:
            continue  # the code is unknown in this program: check_op_codes names it
        kind = "two-qubit channel" if d == 4 else "channel"
        i, c, b = int(i), int(channel[i]), int(branch[i])
        if not 0 <= c < table.shape[0]:
            raise ValueError(f"gate {i}: {kind} index {c} outside 0..{table.shape[0] - 1}")
        m = int(counts[c])
        if not 1 <= m <= d * d:
            raise ValueError(f"gate {i}: {kind} {c} has {m} Kraus matrices (1..{d * d})")
        K = table[c, :m]
        if not np.all(np.isfinite(K)):
            raise ValueError(f"gate {i}: a Kraus matrix of {kind} {c} has an entry that is not finite")
        if not -1 <= b < m:
            raise ValueError(f"gate {i}: branch {b} outside -1..{m - 1}")
        if b < 0:
            dev = float(np.abs(np.einsum("kba,kbc->ac", K.conj(), K) - np.eye(d)).max())
            if not dev <= TRACE_TOL:
                raise ValueError(f"gate {i}: the drawn {kind} {c} is not trace preserving (max |sum K^H K - 1| = {dev:.3e} > {TRACE_TOL:g})")
        if not 0 <= int(q0[i]) < int(n_qubits) - (d == 4):
            raise ValueError(f"gate {i}: {kind} on a qubit outside the register of {int(n_qubits)}")
    return (channel, branch) + tables[OP_K1][1:] + tables[OP_K2][1:]


def check_condition_gates(op, chan, cond_gate, cond_mask):
    """The condition rows of a program, validated: ``(cond_gate int32 [n_gates], cond_mask uint32 [n_gates])``, or ``None`` for a
    program without them or with every gate unconditional.  ``chan`` is what ``check_channel_gates`` returned.  ``ValueError``,
    naming the gate's position, for rows in a program without a channel table, ``cond_mask`` missing, ``cond_gate[i]`` outside
    -1 .. i-1, a gate named that is not of op code 10 or 11, or a mask bit at or above the number of Kraus matrices of that gate's
    channel."""
    if cond_gate is None:
        if cond_mask is not None:
            raise ValueError("a program with cond_mask needs cond_gate")
        return None
    op = np.asarray(op)
    if cond_mask is None:
        raise ValueError("a program with cond_gate needs cond_mask")
    if chan is None:
        raise ValueError("gate 0: condition rows need a program with a channel table")
    cond_gate = np.ascontiguousarray(cond_gate, dtype=np.int32)
    mask = np.asarray(cond_mask)
    if mask.shape != op.shape or cond_gate.shape != op.shape:
        raise ValueError(f"cond_gate and cond_mask must hold one entry per gate ({op.shape[0]}); got shapes {cond_gate.shape}, {mask.shape}")
    if mask.size and (np.any(mask.astype(np.int64) < 0) or np.any(mask.astype(np.int64) > 0xFFFFFFFF)):
        raise ValueError("cond_mask must hold uint32 values")
    mask = np.ascontiguousarray(mask.astype(np.uint32))
    for i in np.flatnonzero(cond_gate != -1):
        i, g = int(i), int(cond_gate[i])
        if not -1 <= g < i:
            raise ValueError(f"gate {i}: condition on gate {g} outside -1..{i - 1}")
        if int(op[g]) not in _CHANNEL:
            raise ValueError(f"gate {i}: condition on gate {g}, which is no channel gate (op code {int(op[g])})")
        counts = chan[3] if int(op[g]) == OP_K1 else chan[5]
        m = int(counts[int(chan[0][g])])
        if int(mask[i]) >> m:
            raise ValueError(f"gate {i}: condition mask names a branch at or above the {m} of gate {g}")
    return (cond_gate, mask) if np.any(cond_gate >= 0) else None


def _condition_mask(values, where) -> int:
    """The mask of the ``values`` of a gate-list condition: an int or an iterable of ints (empty: never)."""
    try:
        vals = [values] if np.ndim(values) == 0 else list(values)
        ok = all(int(v) == v and 0 <= int(v) < 32 for v in vals)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{where}: the values of a condition must be branches 0..31, got {values!r}")
    mask = 0
    for v in vals:
        mask |= 1 << int(v)
    return mask


def _split_gate(g, where):
    """``(name, qubits, params, condition or None)`` of a gate-list entry of three or four elements."""
    if len(g) == 3:
        return g[0], g[1], g[2], None
    if len(g) != 4:
        raise ValueError(f"{where}: a gate is (name, qubits, params[, (g, values)]), got {len(g)} elements")
    cond = g[3]
    if cond is None:
        return g[0], g[1], g[2], None
    try:
        at, values = cond
        at = int(at)
    except (TypeError, ValueError):
        raise ValueError(f"{where}: a condition is (g, values), got {cond!r}") from None
    return g[0], g[1], g[2], (at, _condition_mask(values, where))


class _Conditions:
    """The condition rows of a program under construction from a gate list: ``core[p]`` is the program position of the core op of
    list gate p when that is a channel gate; a routed gate carries its condition on every op it expands to."""

    def __init__(self):
        self.core, self.gate, self.mask, self.any = {}, [], [], False

    def resolve(self, pos, cond):
        """(cond_gate, cond_mask) of list gate ``pos`` with the condition ``cond`` = (list position, mask) or None."""
        if cond is None:
            return -1, 0
        g, mask = cond
        if not 0 <= g < pos:
            raise ValueError(f"gate {pos}: condition on gate {g} outside 0..{pos - 1}")
        if g not in self.core:
            raise ValueError(f"gate {pos}: condition on gate {g}, which is no channel gate")
        self.any = True
        return self.core[g], mask

    def add(self, pos, route_len, core_at, is_channel, cg, cm):
        """List gate ``pos`` takes ``route_len`` ops from here on, its core op being the ``core_at``-th of them."""
        if is_channel:
            self.core[pos] = len(self.gate) + core_at
        self.gate.extend([cg] * route_len), self.mask.extend([cm] * route_len)

    def arrays(self):
        if not self.any:
            return None, None
        return np.asarray(self.gate, dtype=np.int32), np.asarray(self.mask, dtype=np.uint32)


def reject_channels(circuits, what) -> None:
    """``ValueError`` if one of ``circuits`` holds a drawn channel gate: ``what`` builds its states without a seed, state indices
    and trajectories, so every state would draw as state 0 (or as its position in a rank's share) of trajectory 0.  Forced
    branches (``Project``, ``PostSelect`` and their two-qubit forms) draw nothing and pass."""
    for c in circuits:
        k = np.isin(np.asarray(c.op), _CHANNEL)
        if k.any() and (c.branch is None or np.any(np.asarray(c.branch)[k] < 0)):
            raise ValueError(f"{what}: the circuit holds drawn Kraus channels (op codes 10, 11), which this path would run without a seed, state indices and "
                             f"trajectories; use build_noisy_kernel_matrix / build_noisy_projected_kernel_matrix, or simulate / Context.build_mps_set with them")


def entanglement_graph(nq: int, nn: int) -> list[tuple[int, int]]:
    """Linear entanglement map with interactions up to distance ``nn``.

    Same edge set and layer structure as /root/reference/main.py:21-45: for each
    distance, a first layer of disjoint pairs, then the pairs that start on a
    right end of the first layer.
    """
    edges = []
    for dist in range(1, nn + 1):
        taken = np.zeros(nq + dist, dtype=bool)
        second = []
        for left in range(nq - dist):
            if taken[left]:
                second.append(left)
            else:
                edges.append((left, left + dist))
                taken[left + dist] = True
        # qubits that were right ends of the first layer and still have a partner
        edges.extend((left, left + dist) for left in second)
    return edges


@dataclass(frozen=True)
class BoundCircuit:
    """A gate program with numeric angles: what ``circuit_for_data`` returns."""

    n_qubits: int
    op: np.ndarray  # int8   [n_gates]
    q0: np.ndarray  # int32  [n_gates]   (for 2-qubit gates the pair is (q0, q0+1))
    alpha: np.ndarray  # float64 [n_gates] half-turns (0 where unused)
    mat: np.ndarray | None = None  # int32 [n_gates] index into mats of a matrix gate (op 8, 9), -1 at the named gates
    mats: np.ndarray | None = None  # complex128 [n_mats, 4, 4]: the matrix table (a 2x2 sits in [:2, :2], the rest of its slot 0)
    channel: np.ndarray | None = None  # int32 [n_gates] index into kraus (op 10) or kraus2 (op 11) of a channel gate, -1 elsewhere
    branch: np.ndarray | None = None  # int32 [n_gates] -1: the branch is drawn; k >= 0: branch k is forced (read where op is 10 or 11)
    kraus: np.ndarray | None = None  # complex128 [n_channels, 4, 2, 2]: the channel table, K[s'][s] = <s'|K|s>
    n_kraus: np.ndarray | None = None  # int32 [n_channels] Kraus matrices of each channel (1..4)
    kraus2: np.ndarray | None = None  # complex128 [n_channels2, 16, 4, 4]: the two-qubit channel table, K[(p,p')][(s,s')], q0 most significant
    n_kraus2: np.ndarray | None = None  # int32 [n_channels2] Kraus matrices of each two-qubit channel (1..16)
    cond_gate: np.ndarray | None = None  # int32 [n_gates] -1: unconditional; g < i: the channel gate whose recorded branch decides whether gate i runs
    cond_mask: np.ndarray | None = None  # uint32 [n_gates] bit v: branch v of gate cond_gate[i] lets gate i run (read where cond_gate[i] >= 0)

    @property
    def n_channel_gates(self) -> int:
        return int(np.count_nonzero(np.isin(np.asarray(self.op), _CHANNEL)))

    def _with(self, op, q0, alpha, mat, channel, branch, cond_gate=None, cond_mask=None) -> "BoundCircuit":
        return BoundCircuit(self.n_qubits, op, q0, alpha, mat, self.mats, channel, branch, self.kraus, self.n_kraus, self.kraus2, self.n_kraus2, cond_gate, cond_mask)

    def with_branches(self, branches) -> "BoundCircuit":
        """The same program with the branch of its j-th channel gate forced to ``branches[j]`` (-1 leaves it drawn): what replays
        the recorded ``branches`` of a trajectory.  -2 (the gate was skipped: its condition was false) keeps the program's own entry:
        the replay skips the gate again, as the branches its condition reads are replayed too."""
        b = np.asarray(branches, dtype=np.int32).ravel()
        at = np.flatnonzero(np.isin(np.asarray(self.op), _CHANNEL))
        if b.shape[0] != at.shape[0]:
            raise ValueError(f"the program has {at.shape[0]} channel gates, got {b.shape[0]} branches")
        row = np.full(self.op.shape, -1, dtype=np.int32)
        own = np.full(at.shape, -1, dtype=np.int32) if self.branch is None else np.asarray(self.branch, dtype=np.int32)[at]
        row[at] = np.where(b == -2, own, b)
        return self._with(self.op, self.q0, self.alpha, self.mat, self.channel, row, self.cond_gate, self.cond_mask)

    @property
    def n_gates(self) -> int:
        return int(self.op.shape[0])

    def as_tuples(self):
        """(name, qubits, params) triples in the shape of the reference's CPU gate list
        (/root/reference/cpu_backend/kernel_state_ansatz.py:113-131).  A drawn channel gate comes out as ``Kraus1q`` (``Kraus2q``
        for code 11) with all its matrices; one with a forced branch b (``Project``, ``PostSelect``, a replay) as ``Project``
        (``Project2q``) with the one matrix K_b, which gives the same state and ``logw`` when read back (its recorded branch is then
        0, the only one ``Project`` has).  A conditional gate comes out as the 4-tuple ``(name, qubits, params, (g, values))``, g the
        position in this list (one tuple per op) of the gate its condition reads; a condition on a gate that comes out as
        ``Project`` / ``Project2q`` (forced branch b) reads ``[0]`` where bit b of the mask is set and ``[]`` where it is not."""
        chan = check_channel_gates(self.op, self.q0, self.n_qubits, self.channel, self.branch, self.kraus, self.n_kraus, self.kraus2, self.n_kraus2)
        cond = check_condition_gates(self.op, chan, self.cond_gate, self.cond_mask)
        mat, mats = check_matrix_gates(self.op, self.mat, self.mats, with_channels=chan is not None and chan[2] is not None,
                                       with_channels2=chan is not None and chan[4] is not None)
        out = []
        for i, (o, q, a) in enumerate(zip(self.op.tolist(), self.q0.tolist(), self.alpha.tolist())):
            qubits = [q, q + 1] if is_two_qubit(o) else [q]
            if o in _CHANNEL:  # drawn: ("Kraus1q", [q], [[K0, ..]]); forced: ("Project", [q], [K_b]), the same state and logw
                c, b = int(chan[0][i]), int(chan[1][i])
                table, counts = (chan[2], chan[3]) if o == OP_K1 else (chan[4], chan[5])
                if b >= 0:
                    out.append(("Project" if o == OP_K1 else "Project2q", qubits, [table[c, b].copy()]))
                else:
                    out.append((_OP_NAMES[o], qubits, [table[c, : int(counts[c])].copy()]))
            elif o in _MATRIX:  # ("Unitary1q", [q], [M2x2]) / ("Unitary2q", [q, q+1], [M4x4])
                d = 2 if o == OP_M1 else 4
                out.append((_OP_NAMES[o], qubits, [mats[mat[i], :d, :d].copy()]))
            else:
                out.append((_OP_NAMES[o], qubits, [a] if o in _PARAMETRISED else []))
            if cond is not None and cond[0][i] >= 0:
                g, mask = int(cond[0][i]), int(cond[1][i])
                forced = int(chan[1][g])
                values = [v for v in range(32) if (mask >> v) & 1] if forced < 0 else ([0] if (mask >> forced) & 1 else [])
                out[-1] = out[-1] + ((g, values),)
        return out

    def sliced(self, a, b) -> "BoundCircuit":
        """The same qubits with gates a .. b-1 of the program (0 <= a <= b <= n_gates): ``sliced(0, c)`` is the circuit a checkpoint
        at c gates has run, ``sliced(c, n_gates)`` what a build resumed from that snapshot still has to run."""
        a, b = int(a), int(b)
        if not 0 <= a <= b <= self.n_gates:
            raise ValueError(f"sliced({a}, {b}): want 0 <= a <= b <= {self.n_gates} gates")
        cut = lambda v: None if v is None else v[a:b]  # noqa: E731
        cg, cm = cut(self.cond_gate), cut(self.cond_mask)
        if cg is not None:  # positions are relative to the program of a call: a kept gate may read kept gates only
            cg = np.asarray(cg, dtype=np.int32)
            behind = np.flatnonzero((cg >= 0) & (cg < a))
            if behind.size:
                raise ValueError(f"sliced({a}, {b}): gate {a + int(behind[0])} is conditioned on gate {int(cg[behind[0]])}, which lies in front of the slice")
            cg = np.where(cg >= 0, cg - a, cg).astype(np.int32)
        return self._with(self.op[a:b], self.q0[a:b], self.alpha[a:b], cut(self.mat), cut(self.channel), cut(self.branch), cg, cm)

    @classmethod
    def from_gates(cls, n_qubits, gates, named_constants: bool = False) -> "BoundCircuit":
        """A gate list in the shape of the reference's CPU backend -- ``(name, qubits, params)`` with the names of
        ``_OP_NAMES`` and ``params`` the half-turn angle in a one-element list (empty for H and SWAP) -- as a program.
        A two-qubit gate on non-adjacent or reversed qubits is routed like KernelStateAnsatz's XXPhase: SWAP chain up,
        the gate on (hi-1, hi), the chain back.  The named two-qubit rotations and SWAP are symmetric in their qubits; a matrix
        gate need not be: on qubits ``[a, b]`` with a > b the matrix is applied with the two qubit roles exchanged
        (``exchange_qubits``), so ``("CX", [3, 2], [])`` has its control on qubit 3.

        Classical control: a gate may carry a fourth element ``(g, values)``: g is the list position of an earlier channel gate
        (code 10 or 11), ``values`` an int or an iterable of ints, the branches of that gate that let this one run (empty: never).
        A routed gate carries the condition on every op it expands to; g is mapped to the program position of the core op.

        Matrix gates: ``("Unitary1q", [q], [M])`` and ``("Unitary2q", [a, b], [M])`` with M a unitary 2x2 / 4x4 (index (s_a, s_b),
        a most significant), and -- with ``named_constants=True`` -- the named constants X, Y, Z, S, Sdg, T, Tdg, V, Vdg, SX, SXdg,
        CX, CY, CZ (control first) without parameters.  The constants are opt-in here because the vocabulary of a plain
        ``from_gates(n, gates)`` is pinned to the op-code names (any other name, CX included, stays the ``ValueError`` it has always
        been); ``as_bound_circuit`` -- the way a gate-list ansatz enters ``build_kernel_matrix`` and the builder pools -- and
        ``CircuitAnsatz`` templates take them without asking.

        Table slots are assigned by structure only: every explicit unitary gets its own slot in order of appearance,
        a named constant one slot per name (and, for CX and CY, per orientation) at its first use -- so the circuits of the data
        points of one gate-list ansatz share ``op``, ``q0`` and ``mat`` and differ in ``alpha`` and ``mats``.  ``ValueError`` for a
        matrix of the wrong shape or one that is not unitary to UNITARY_TOL."""
        n = int(n_qubits)
        op, q0, alpha, mat, channel, branch = [], [], [], [], [], []
        table, chans, chans2, conds = _MatTable(), _ChannelTable(), _ChannelTable(4), _Conditions()
        for pos, g in enumerate(gates):
            name, qubits, params, cond = _split_gate(g, f"gate {pos}")
            code = _gate_code(name, named_constants)
            qubits = [int(q) for q in qubits]
            if _arity(code) != len(qubits):
                raise ValueError(f"{name} acts on {_arity(code)} qubit(s), got {qubits}")
            cg, cm = conds.resolve(pos, cond)
            if code == OP_K1:
                if not 0 <= qubits[0] < n:
                    raise ValueError(f"gate on qubits {qubits} outside a register of {n}")
                slot, forced = chans.slot(name, params, f"gate {pos}")
                conds.add(pos, 1, 0, True, cg, cm)
                op.append(OP_K1), q0.append(qubits[0]), alpha.append(0.0), mat.append(-1), channel.append(slot), branch.append(forced)
                continue
            if code == OP_K2:  # routed like a matrix gate; on [a, b] with a > b the matrices go in with the qubit roles exchanged
                route = _route(code, qubits, n)
                slot, forced = chans2.slot(name, params, f"gate {pos}", exchange=qubits[0] > qubits[1])
                conds.add(pos, len(route), len(route) // 2, True, cg, cm)
                for o, q, k in route:
                    op.append(o), q0.append(q), alpha.append(0.0), mat.append(-1), channel.append(slot if k else -1), branch.append(forced if k else -1)
                continue
            if code in _MATRIX:
                if name in _NAMED:
                    if params is not None and np.size(params) != 0:
                        raise ValueError(f"{name}: expected 0 parameter(s), got {list(params)}")
                    params = None
                slot = table.slot(name, qubits, params, f"gate {pos}")
                route = _route(code, qubits, n)
                conds.add(pos, len(route), 0, False, cg, cm)
                for o, q, k in route:
                    op.append(o), q0.append(q), alpha.append(0.0), mat.append(slot if k else -1), channel.append(-1), branch.append(-1)
                continue
            if params is None:
                params = []
            elif np.ndim(params) == 0:
                params = [params]
            if len(params) != (1 if code in _PARAMETRISED else 0):
                raise ValueError(f"{name}: expected {1 if code in _PARAMETRISED else 0} parameter(s), got {list(params)}")
            a = float(params[0]) if params else 0.0
            route = _route(code, qubits, n)
            conds.add(pos, len(route), 0, False, cg, cm)
            for o, q, k in route:
                op.append(o), q0.append(q), alpha.append(a if k else 0.0), mat.append(-1), channel.append(-1), branch.append(-1)
        core = (n, np.asarray(op, dtype=np.int8), np.asarray(q0, dtype=np.int32), np.asarray(alpha, dtype=np.float64))
        mt = (np.asarray(mat, dtype=np.int32), table.array()) if table.entries else (None, None)
        if not chans.entries and not chans2.entries:
            return cls(*core) if not table.entries else cls(*core, *mt)
        rows = (np.asarray(channel, dtype=np.int32), np.asarray(branch, dtype=np.int32))
        return cls(*core, *mt, *rows, *(chans.arrays() if chans.entries else (None, None)), *(chans2.arrays() if chans2.entries else (None, None)), *conds.arrays())


def check_checkpoints(checkpoints, n_gates) -> list:
    """The checkpoints of a scan build as a list of ints, or ``ValueError``: gate counts, strictly increasing, each in 1 .. n_gates,
    the last one ``n_gates`` (the finished circuit is always the last snapshot)."""
    try:
        cps = [int(c) for c in checkpoints]
        exact = all(c == k for c, k in zip(checkpoints, cps))
    except (TypeError, ValueError):
        raise ValueError(f"checkpoints must be a list of gate counts, got {checkpoints!r}") from None
    if not cps:
        raise ValueError("checkpoints is empty: a scan needs at least the finished circuit")
    if not exact or any(not 1 <= c <= int(n_gates) for c in cps):
        raise ValueError(f"checkpoints must be ints in 1 .. {int(n_gates)} (gates done), got {list(checkpoints)!r}")
    if any(b <= a for a, b in zip(cps, cps[1:])):
        raise ValueError(f"checkpoints must be strictly increasing, got {cps!r}")
    if cps[-1] != int(n_gates):
        raise ValueError(f"the last checkpoint must be the whole program ({int(n_gates)} gates), got {cps[-1]}")
    return cps


def check_depths(depths, reps) -> list:
    """The depths of a depth scan as a list of ints, or ``ValueError``: distinct, each in 1 .. ``reps``."""
    try:
        ds = list(depths)
    except TypeError:
        raise ValueError(f"depths must be a list of layer counts, got {depths!r}") from None
    if not ds or any(isinstance(d, bool) or not isinstance(d, (int, np.integer)) or not 1 <= d <= int(reps) for d in ds) or len(set(ds)) != len(ds):
        raise ValueError(f"depths must be distinct ints in 1 .. reps = {int(reps)}, got {ds!r}")
    return [int(d) for d in ds]


def _arity(o) -> int:
    return 2 if is_two_qubit(o) else 1


def _gate_code(name, named_constants: bool = True) -> int:
    if isinstance(name, str) and name in _CHANNEL_NAMES:
        return OP_K1
    if isinstance(name, str) and name in _CHANNEL2_NAMES:
        return OP_K2
    if isinstance(name, str) and name in _NAMED:
        if not named_constants:
            also = f"from_gates(..., named_constants=True) also takes {', '.join(_NAMED)}"
            raise ValueError(f"unknown gate {name!r} (supported: {', '.join(_OP_CODES)}; {also})")
        return OP_M1 if name in _NAMED_1Q else OP_M2
    try:
        return _OP_CODES[name]
    except (KeyError, TypeError):
        raise ValueError(f"unknown gate {name!r} (supported: {', '.join(list(_OP_CODES) + list(_NAMED))})") from None


class _MatTable:
    """The matrix table of a program under construction: slots by structure only (see ``BoundCircuit.from_gates``)."""

    def __init__(self):
        self.entries, self._named = [], {}

    def slot(self, name, qubits, params, where) -> int:
        """The table slot of one matrix gate as given (unrouted): ``params`` is ``None`` for a named constant, else the matrix (or
        a one-element list holding it).  On reversed qubits the 4x4 goes in with its qubit roles exchanged."""
        d = 2 if len(qubits) == 1 else 4
        reverse = d == 4 and qubits[0] > qubits[1]
        if name in _NAMED:
            m = np.array(_NAMED[name], dtype=np.complex128)
            key = (name, bool(reverse and not np.array_equal(exchange_qubits(m), m)))
            if key in self._named:
                return self._named[key]
        else:
            try:
                m = np.asarray(params, dtype=np.complex128)
            except (TypeError, ValueError):
                raise ValueError(f"{where} ({name}): the parameter must be one {d}x{d} complex matrix") from None
            if m.shape == (1, d, d):
                m = m[0]
            if m.shape != (d, d):
                raise ValueError(f"{where} ({name}): expected one {d}x{d} matrix, got shape {m.shape}")
            check_unitary(m, f"{where} ({name})")
            key = None
        full = np.zeros((4, 4), dtype=np.complex128)
        full[:d, :d] = exchange_qubits(m) if reverse else m
        self.entries.append(full)
        if key is not None:
            self._named[key] = len(self.entries) - 1
        return len(self.entries) - 1

    def array(self) -> np.ndarray:
        return np.stack(self.entries) if self.entries else np.zeros((0, 4, 4), dtype=np.complex128)


def _route(code, qubits, n):
    """The adjacent-pair program of one gate: [(op, q0, is_the_gate)].  A two-qubit gate on (a, b) becomes a SWAP chain
    bringing min(a, b) next to max(a, b), the gate on (hi-1, hi), and the chain back (KernelStateAnsatz's routing)."""
    if not all(0 <= q < n for q in qubits):
        raise ValueError(f"gate on qubits {qubits} outside a register of {n}")
    if not is_two_qubit(code):
        return [(code, qubits[0], True)]
    a, b = qubits
    if a == b:
        raise ValueError(f"two-qubit gate on ({a}, {b})")
    lo, hi = (a, b) if a < b else (b, a)
    return ([(OP_SWAP, q, False) for q in range(lo, hi - 1)] + [(code, hi - 1, True)]
            + [(OP_SWAP, q, False) for q in range(hi - 2, lo - 1, -1)])


def as_bound_circuit(circuit, ansatz) -> BoundCircuit:
    """What ``ansatz.circuit_for_data`` returned, as a program: a reference-style gate list ``(name, qubits, params)``
    through ``BoundCircuit.from_gates`` (named constants included) with ``n_qubits`` from ``ansatz.ansatz_circ.n_qubits``
    (as reference G:147); a BoundCircuit as it is."""
    if isinstance(circuit, (list, tuple)):
        return BoundCircuit.from_gates(ansatz.ansatz_circ.n_qubits, circuit, named_constants=True)
    return circuit


class GateProgram:
    """The symbolic (unbound) circuit; stands in for the reference's ``ansatz_circ``."""

    def __init__(self, n_qubits, op, q0, fa, fb, scale):
        self.n_qubits = int(n_qubits)
        self.op, self.q0, self.fa, self.fb, self.scale = op, q0, fa, fb, scale

    @property
    def n_gates(self) -> int:
        return int(self.op.shape[0])

    def bind(self, x: np.ndarray) -> BoundCircuit:
        alpha = np.zeros(self.op.shape[0])
        rz = self.op == OP_RZ
        xx = self.op == OP_XX
        alpha[rz] = self.scale[rz] * x[self.fa[rz]]
        alpha[xx] = self.scale[xx] * (1.0 - x[self.fa[xx]]) * (1.0 - x[self.fb[xx]])
        return BoundCircuit(self.n_qubits, self.op, self.q0, alpha)


class KernelStateAnsatz:
    """Drop-in for the reference class of the same name (ref :16-103).

    Attributes kept from the reference: ``ansatz_circ`` (needs ``.n_qubits``,
    used at ref :147) and ``feature_symbol_list`` (names ``f_0 .. f_{n-1}``).
    """

    def __init__(self, num_qubits, reps, gamma, entanglement_map, hadamard_init=True):
        n = int(num_qubits)
        self.num_qubits, self.reps, self.gamma = n, int(reps), float(gamma)
        self.entanglement_map = [(int(a), int(b)) for a, b in entanglement_map]
        self.hadamard_init = bool(hadamard_init)
        self.feature_symbol_list = [f"f_{i}" for i in range(n)]
        self.one_q_symbol_list = []
        self.two_q_symbol_list = []

        op, q0, fa, fb, sc = [], [], [], [], []

        def emit(o, q, a=0, b=0, s=0.0):
            op.append(o), q0.append(q), fa.append(a), fb.append(b), sc.append(s)

        if self.hadamard_init:
            for q in range(n):
                emit(OP_H, q)
        rz_scale = (2.0 / np.pi) * self.gamma
        xx_scale = self.gamma * self.gamma
        for _ in range(self.reps):
            for q in range(n):
                emit(OP_RZ, q, q, 0, rz_scale)
            for a, b in self.entanglement_map:
                if not (0 <= a < n and 0 <= b < n) or a == b:
                    raise ValueError(f"bad entanglement pair ({a}, {b}) for {n} qubits")
                lo, hi = (a, b) if a < b else (b, a)
                for q in range(lo, hi - 1):  # bring qubit `lo` next to `hi`
                    emit(OP_SWAP, q)
                emit(OP_XX, hi - 1, a, b, xx_scale)
                for q in range(hi - 2, lo - 1, -1):  # and back
                    emit(OP_SWAP, q)
        self._n_head = n if self.hadamard_init else 0
        self.ansatz_circ = GateProgram(
            n,
            np.asarray(op, dtype=np.int8),
            np.asarray(q0, dtype=np.int32),
            np.asarray(fa, dtype=np.int32),
            np.asarray(fb, dtype=np.int32),
            np.asarray(sc, dtype=np.float64),
        )

    def layer_ends(self) -> list:
        """Gate counts after layers 1 .. reps: ``[n_h + r L]`` with n_h the Hadamards in front and L the gates of one layer.  The
        ansatz emits the same layer ``reps`` times, so the first ``layer_ends()[r - 1]`` gates of a bound circuit ARE the bound
        circuit of the ansatz with r layers: the checkpoints of a depth scan."""
        total = self.ansatz_circ.n_gates
        per_layer = (total - self._n_head) // self.reps if self.reps > 0 else 0
        return [self._n_head + r * per_layer for r in range(1, self.reps + 1)]

    def circuit_for_data(self, feature_values) -> BoundCircuit:
        """Bind one data point.  ``RuntimeError`` on a length mismatch, as ref :96-97."""
        if len(feature_values) != len(self.feature_symbol_list):
            raise RuntimeError("The number of values must match the number of symbols.")
        return self.ansatz_circ.bind(np.asarray(feature_values, dtype=np.float64))


class CircuitProgram:
    """The compiled (unbound) gate program of a ``CircuitAnsatz``: per routed gate an op code, a pair / qubit and the
    angle form alpha = s (c_a + d_a x[a]) (c_b + d_b x[b]) (s = 0 for H and SWAP; c = 1, d = 0 for an absent factor)."""

    def __init__(self, n_qubits, op, q0, s, fa, ca, da, fb, cb, db, mat=None, mats=None, channel=None, branch=None, kraus=None, n_kraus=None, kraus2=None,
                 n_kraus2=None, cond_gate=None, cond_mask=None):
        self.n_qubits = int(n_qubits)
        self.op, self.q0 = op, q0
        self.s, self.fa, self.ca, self.da, self.fb, self.cb, self.db = s, fa, ca, da, fb, cb, db
        self.mat, self.mats = mat, mats  # constant matrix gates: the table is the same array for every data point
        self.channel, self.branch, self.kraus, self.n_kraus = channel, branch, kraus, n_kraus  # channels are constants of the ansatz too
        self.kraus2, self.n_kraus2 = kraus2, n_kraus2
        self.cond_gate, self.cond_mask = cond_gate, cond_mask  # classical control is gate structure: the same for every data point

    @property
    def n_gates(self) -> int:
        return int(self.op.shape[0])

    def bind(self, x: np.ndarray) -> BoundCircuit:
        alpha = self.s * (self.ca + self.da * x[self.fa]) * (self.cb + self.db * x[self.fb])
        return BoundCircuit(self.n_qubits, self.op, self.q0, alpha, self.mat, self.mats, self.channel, self.branch, self.kraus, self.n_kraus, self.kraus2, self.n_kraus2,
                            self.cond_gate, self.cond_mask)


def _factor(spec, n_features):
    a, c, d = spec
    if not 0 <= int(a) < n_features:
        raise ValueError(f"feature index {a} outside 0..{n_features - 1}")
    return int(a), float(c), float(d)


class CircuitAnsatz:
    """A custom feature map: a gate template compiled once, bound per data point by one vectorised expression.

    ``gates`` is a list of ``(name, qubits, angle)`` with the names of ``BoundCircuit.from_gates`` (H, Rz, Rx, Ry, XXPhase,
    YYPhase, ZZPhase, SWAP), angles in half-turns (theta = pi alpha / 2).  ``angle`` is
      * ``None`` for H and SWAP;
      * a number: a constant angle;
      * ``(s, (a, c_a, d_a))``: alpha = s (c_a + d_a x[a]);
      * ``(s, (a, c_a, d_a), (b, c_b, d_b))``: alpha = s (c_a + d_a x[a]) (c_b + d_b x[b]).
    The reference ansatz is Rz ``((2/pi) gamma, (i, 0, 1))`` and XXPhase ``(gamma^2, (a, 1, -1), (b, 1, -1))``; a
    Havlicek-style ZZ map is ZZPhase ``(s, (a, pi, -1), (b, pi, -1))``.  Two-qubit gates on non-adjacent or reversed
    qubits are routed as in ``BoundCircuit.from_gates``.  Constant matrix gates: the named constants of ``from_gates`` (X, Y, Z, S,
    Sdg, T, Tdg, V, Vdg, SX, SXdg, CX, CY, CZ) with angle ``None``, and ``("Unitary1q" | "Unitary2q", qubits, M)`` with a constant
    unitary M in the place of the angle; every data point shares the one table.  A gate may carry a fourth element ``(g, values)``,
    the condition of ``from_gates``: it runs only where the channel gate at list position g took one of ``values``.  ``num_features`` defaults to ``num_qubits``
    (one feature per qubit, as the reference's ``feature_symbol_list``).  Picklable: plain numpy arrays only."""

    def __init__(self, num_qubits, gates, num_features=None):
        n = int(num_qubits)
        nf = n if num_features is None else int(num_features)
        if nf < 1:
            raise ValueError("a feature map needs at least one feature")
        self.num_qubits, self.num_features = n, nf
        self.feature_symbol_list = [f"f_{i}" for i in range(nf)]
        cols = {k: [] for k in ("op", "q0", "s", "fa", "ca", "da", "fb", "cb", "db")}
        mat, table = [], _MatTable()
        channel, branch, chans, chans2, conds = [], [], _ChannelTable(), _ChannelTable(4), _Conditions()
        for pos, g in enumerate(gates):
            name, qubits, angle, cond = _split_gate(g, f"gate {pos}")
            code = _gate_code(name)
            qubits = [int(q) for q in (qubits if np.ndim(qubits) else [qubits])]
            if _arity(code) != len(qubits):
                raise ValueError(f"{name} acts on {_arity(code)} qubit(s), got {qubits}")
            one = (0, 1.0, 0.0)
            slot, cslot, forced = -1, -1, -1
            if code == OP_K1:  # the channel's parameters stand in the place of the angle: constants of the ansatz
                cslot, forced = chans.slot(name, angle, f"gate {pos}")
                s, fa, fb = 0.0, one, one
            elif code == OP_K2:
                if len(set(qubits)) == 2:  # (a pair on one qubit is refused by the routing below)
                    cslot, forced = chans2.slot(name, angle, f"gate {pos}", exchange=qubits[0] > qubits[1])
                s, fa, fb = 0.0, one, one
            elif code in _MATRIX:
                if name in _NAMED and angle is not None:
                    raise ValueError(f"{name} takes no angle, got {angle!r}")
                slot = table.slot(name, qubits, angle, f"gate {pos}")
                s, fa, fb = 0.0, one, one
            elif code not in _PARAMETRISED:
                if angle is not None:
                    raise ValueError(f"{name} takes no angle, got {angle!r}")
                s, fa, fb = 0.0, one, one
            elif angle is None:
                raise ValueError(f"{name} needs an angle")
            elif not isinstance(angle, (tuple, list)):
                s, fa, fb = float(angle), one, one
            else:
                if len(angle) not in (2, 3):
                    raise ValueError(f"{name}: angle {angle!r} is not (s, (a, c_a, d_a)[, (b, c_b, d_b)])")
                s, fa = float(angle[0]), _factor(angle[1], nf)
                fb = _factor(angle[2], nf) if len(angle) == 3 else one
            route = _route(code, qubits, n)
            conds.add(pos, len(route), len(route) // 2, code in _CHANNEL, *conds.resolve(pos, cond))
            for o, q, is_gate in route:
                row = (o, q, s, *fa, *fb) if is_gate else (o, q, 0.0, *one, *one)
                for k, v in zip(cols, row):
                    cols[k].append(v)
                mat.append(slot if is_gate else -1)
                channel.append(cslot if is_gate else -1), branch.append(forced if is_gate else -1)
        dt = {"op": np.int8, "q0": np.int32, "fa": np.int32, "fb": np.int32}
        arr = {k: np.asarray(v, dtype=dt.get(k, np.float64)) for k, v in cols.items()}
        if table.entries:
            arr["mat"], arr["mats"] = np.asarray(mat, dtype=np.int32), table.array()
        if chans.entries or chans2.entries:
            arr["channel"], arr["branch"] = np.asarray(channel, dtype=np.int32), np.asarray(branch, dtype=np.int32)
        if chans.entries:
            arr["kraus"], arr["n_kraus"] = chans.arrays()
        if chans2.entries:
            arr["kraus2"], arr["n_kraus2"] = chans2.arrays()
        if conds.any:
            arr["cond_gate"], arr["cond_mask"] = conds.arrays()
        self.ansatz_circ = CircuitProgram(n, **arr)

    def layer_ends(self) -> list:
        """A custom gate template has no layer structure of its own: one entry, the whole program.  A scan build
        (``Context.build_mps_scan``, ``simulate(..., checkpoints=)``) takes any gate counts as checkpoints."""
        return [self.ansatz_circ.n_gates]

    def circuit_for_data(self, feature_values) -> BoundCircuit:
        """Bind one data point.  ``RuntimeError`` on a length mismatch, as reference G:96-97."""
        if len(feature_values) != len(self.feature_symbol_list):
            raise RuntimeError("The number of values must match the number of symbols.")
        return self.ansatz_circ.bind(np.asarray(feature_values, dtype=np.float64))
