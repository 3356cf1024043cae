"""Matrix-product states: the container that crosses the hot-path boundary, and the
host-side builder that produces the path's inputs.

``MPS`` mirrors what the reference uses of pytket-cutensornet's MPS object
(/root/reference/gpu_backend/kernel_state_ansatz.py:223,290,295-296,370,374,380):
``tensors``, ``get_virtual_dimensions``, ``fidelity``, ``copy``,
``update_libhandle``, ``len`` and ``vdot``.  Site tensors are complex128 numpy
arrays indexed ``[left bond, physical, right bond]``.

``simulate`` is the *input producer* (SURVEY.md section 8, row A8 / N1), not the hot
path: it applies the bound gate program to |0...0> gate by gate with one SVD per
two-qubit gate, truncating at ``truncation_fidelity`` exactly where the reference
does (ref :141-144, :221; criterion as ITensors ``cutoff``,
/root/reference/KernelPkg/src/KernelPkg.jl:68).  It runs on the host (LAPACK); a
device builder is the next row of the scope table.
"""
from __future__ import annotations

import os

import numpy as np
from scipy.linalg import qr as _qr
from scipy.linalg import svd as _svd

from . import program as _program
from .ansatz import (OP_H, OP_K1, OP_K2, OP_M1, OP_M2, OP_RX, OP_RZ, OP_SWAP, OP_YY, OP_ZZ, BoundCircuit, check_channel_gates, check_checkpoints, check_condition_gates, check_matrix_gates,
                     is_two_qubit, reject_channels)

_SQRT_HALF = 0.7071067811865476
_YY_SIGN = np.array([[1.0, -1.0], [-1.0, 1.0]])[None, :, :, None]  # c 1 - i s Y(x)Y: +i s on |00>,|11>, -i s on |01>,|10>


class MPS:
    """n-site matrix-product state, open boundaries, physical dimension 2."""

    __slots__ = ("tensors", "fidelity", "logw", "branches", "_handle")

    def __init__(self, tensors, fidelity: float = 1.0, logw: float = 0.0, branches=None):
        self.tensors = list(tensors)
        self.fidelity = float(fidelity)
        # a trajectory of a program with Kraus channels: the log of the probability of its branches, sum log(p_b / N), and the
        # branch of every channel gate in program order (int8; empty for a program without channels)
        self.logw = float(logw)
        self.branches = np.zeros(0, dtype=np.int8) if branches is None else np.asarray(branches, dtype=np.int8).copy()
        self._handle = None
        left = 1
        for k, t in enumerate(self.tensors):
            if t.ndim != 3 or t.shape[1] != 2 or t.shape[0] != left:
                raise RuntimeError(f"site {k}: tensor shape {t.shape} does not chain (left bond {left}, physical 2)")
            left = t.shape[2]
        if left != 1:
            raise RuntimeError("the last right bond must have dimension 1")

    def __len__(self) -> int:
        return len(self.tensors)

    def get_virtual_dimensions(self, position: int) -> tuple[int, int]:
        t = self.tensors[position]
        return (t.shape[0], t.shape[2])

    def bond_dims(self) -> np.ndarray:
        """chi[0..n]: chi[0] = chi[n] = 1."""
        return np.asarray([1] + [t.shape[2] for t in self.tensors], dtype=np.int32)

    def max_bond(self) -> int:
        return int(self.bond_dims().max())

    def nbytes(self) -> int:
        return int(sum(t.nbytes for t in self.tensors))

    def copy(self) -> "MPS":
        return MPS([t.copy() for t in self.tensors], self.fidelity, self.logw, self.branches)

    def update_libhandle(self, handle) -> None:
        """Accepted for interface parity (ref :370,:374); states are immutable host
        arrays here and device residency is owned by the engine's MPS sets."""
        self._handle = handle

    def bond_spectra(self) -> list:
        """Schmidt weights across every interior bond, on the host: a list of n - 1 float64 arrays, entry k - 1 the descending
        weights lambda_k[0 .. chi_k - 1] (sum 1) of the cut between sites k - 1 and k -- the eigenvalues of N_k = R_k L_k^T /
        <psi|psi> that ``Context.bond_spectra`` returns.  By canonicalisation: the chain is right-orthonormalised by QR, then one
        SVD per bond carries the centre to the right; weights below the bond's rank are zero.  Independent of the gauge of the
        bonds and of the norm of the state."""
        n = len(self.tensors)
        ts = [np.asarray(t, dtype=np.complex128) for t in self.tensors]
        for k in range(n - 1, 0, -1):
            l, _, r = ts[k].shape
            q, rr = np.linalg.qr(ts[k].reshape(l, 2 * r).T)  # (2r, l) = q (2r, m) rr (m, l)
            ts[k] = q.T.reshape(-1, 2, r)
            ts[k - 1] = np.tensordot(ts[k - 1], rr.T, axes=(2, 0))
        out = []
        centre = ts[0]
        for k in range(1, n):
            l, _, r = centre.shape
            _, s, vh = np.linalg.svd(centre.reshape(l * 2, r), full_matrices=False)
            w = np.zeros(self.tensors[k].shape[0], dtype=np.float64)
            w[: min(s.size, w.size)] = (s * s)[: w.size] / float((s * s).sum())
            out.append(w)
            centre = np.tensordot(s[:, None] * vh, ts[k], axes=(1, 0))
        return out

    def compress(self, max_bond: int | None = None, max_discard: float = 0.0, value_of_zero: float = 1e-16):
        """The state truncated once, in canonical form: ``(MPS, discarded)``, the host mirror of ``Context.compress``.  The
        ``bond_spectra`` sweep with a cut: the chain is right-orthonormalised from the last site (a bond keeps its singular values
        above ``value_of_zero`` times the Frobenius norm of the site's matrix, so a rank-deficient bond shrinks to its rank), then the centre moves to the right with one
        SVD per bond.  At bond k, with the singular values descending and total = sum sigma^2: values <= ``value_of_zero``
        sqrt(total) go, then the smallest ones while their summed weight stays <= ``max_discard`` total (``_kept``), then whatever
        exceeds ``max_bond``; at least one stays.  What is kept is scaled by sqrt(total / kept), so <psi'|psi'> = <psi|psi>: the norm
        sits in the last site and sites 0 .. n-2 are left isometries.  ``discarded[k - 1]`` = 1 - kept / total at bond k (the
        dropped weights summed from the small end) and ``.fidelity`` of the result is the product of kept / total in bond order --
        which is |<psi|psi'>|^2 / (<psi|psi> <psi'|psi'>), because the projectors of successive bonds are nested."""
        out, discarded, _ = self._compress(max_bond, max_discard, value_of_zero)
        return out, discarded

    def _compress(self, max_bond, max_discard, value_of_zero):
        """``compress`` and, third, the singular values the cut of every bond was made on (descending, before the cut)."""
        cap = 0 if max_bond is None else int(max_bond)
        budget, zero = float(max_discard), float(value_of_zero)
        if cap < 0 or (max_bond is not None and cap != max_bond):
            raise ValueError(f"max_bond must be an int >= 1, or None / 0 for no cap (got {max_bond!r})")
        if not (budget >= 0.0 and np.isfinite(budget)) or not (zero >= 0.0 and np.isfinite(zero)):
            raise ValueError(f"max_discard and value_of_zero must be >= 0 and finite (got {max_discard!r}, {value_of_zero!r})")
        n = len(self.tensors)
        ts = [np.array(t, dtype=np.complex128) for t in self.tensors]
        for k in range(n - 1, 0, -1):
            l, _, r = ts[k].shape
            u, s, vh = np.linalg.svd(ts[k].reshape(l, 2 * r).T, full_matrices=False)  # (2r, l) = u s vh
            total = float((s * s).sum())
            if not total > 0.0:
                raise ValueError("compress: the state has norm 0")
            m = max(int(np.count_nonzero(s > zero * np.sqrt(total))), 1)
            ts[k] = u[:, :m].T.reshape(m, 2, r)
            ts[k - 1] = np.tensordot(ts[k - 1], (s[:m, None] * vh[:m]).T, axes=(2, 0))
        discarded = np.zeros(n - 1, dtype=np.float64)
        fidelity, sigmas = 1.0, []
        for k in range(n - 1):
            l, _, r = ts[k].shape
            u, s, vh = np.linalg.svd(ts[k].reshape(l * 2, r), full_matrices=False)
            w = s * s
            total = float(w.sum())
            sigmas.append(s)
            if not total > 0.0:
                raise ValueError("compress: the state has norm 0")
            m, _ = _kept(s, budget, zero * np.sqrt(total))
            if cap > 0:
                m = min(m, cap)
            d = float(w[m:][::-1].sum()) / total
            discarded[k] = d
            fidelity *= 1.0 - d
            ts[k] = u[:, :m].reshape(l, 2, m)
            ts[k + 1] = np.tensordot((s[:m, None] * vh[:m]) / np.sqrt(1.0 - d), ts[k + 1], axes=(1, 0))
        return MPS(ts, fidelity), discarded, sigmas

    def block_overlap(self, other: "MPS", width: int, side: str = "left") -> float:
        """Overlap of the reduced states of a block at one end of the chain, on the host: ``tr(rho_A(self) rho_A(other))`` with
        ``rho_A(psi) = tr_{not A} |psi><psi| / <psi|psi>`` and A the first ``width`` qubits (``side="left"``) or the last
        (``side="right"``) -- the numpy mirror of ``Context.block_overlaps``.  One environment loop: the mixed left environment
        ``E_w[b][a] = <l^x_a | l^y_b>`` of the fidelity sweep and the self right environments ``R_w`` of both states, then
        ``sum Rx[a][a'] Ry[b][b'] E[b][a'] conj(E[b'][a]) / (<x|x> <y|y>)``.  The right block is the left block of the reversed
        chains.  ``other=self`` gives the purity of the cut; ``width = n`` the normalised fidelity."""
        n = len(self.tensors)
        if len(other) != n:
            raise ValueError("the two MPS must have the same number of sites")
        if isinstance(width, bool) or not isinstance(width, (int, np.integer)) or not 1 <= width <= n:
            raise ValueError(f"width must be an int in 1 .. {n}, got {width!r}")
        if side not in ("left", "right"):
            raise ValueError(f"side must be 'left' or 'right', got {side!r}")
        w = int(width)
        chains = []
        for m in (self, other):
            ts = [np.asarray(t, dtype=np.complex128) for t in m.tensors]
            chains.append([t.transpose(2, 1, 0) for t in reversed(ts)] if side == "right" else ts)
        x, y = chains
        E = np.ones((1, 1), dtype=np.complex128)  # E[b][a]: ket of y, bra of x
        for k in range(w):
            E = np.einsum("ba,bsc,asd->cd", E, y[k], x[k].conj(), optimize=True)
        envs, norms = [], []
        for ts in (x, y):  # R[ket][bra] at bond w, and <psi|psi> = R_0[0][0]
            R = np.ones((1, 1), dtype=np.complex128)
            Rw = R
            for k in range(n - 1, -1, -1):
                R = np.einsum("asc,cd,bsd->ab", ts[k], R, ts[k].conj(), optimize=True)
                if k == w:
                    Rw = R
            envs.append(Rw)
            norms.append(float(R[0, 0].real))
        V = envs[1].T @ E           # V[b'][a'] = sum_b Ry[b][b'] E[b][a']
        W = E.T @ V.conj()          # W[a][a'] = sum_b' E[b'][a] conj(V[b'][a'])
        return float((envs[0] * W.conj()).sum().real) / (norms[0] * norms[1])

    def window_rdm(self, start: int, width: int) -> np.ndarray:
        """Reduced density matrix of the qubits ``start .. start + width - 1`` on the host, complex128 of shape (2^w, 2^w): the numpy
        mirror of ``Context.window_rdms``.  ``rho[s][s'] = sum over all other sites of psi(.. s ..) conj(psi(.. s' ..)) / <psi|psi>``
        with the row index ``s = sum_j s_{start+j} 2^(w-1-j)`` (qubit ``start`` is the most significant bit).  A plain environment
        loop: L_a and R_b in the X[ket][bra] orientation, the product M^s of the window's sites, then
        ``sum L_a[al][al'] M^s[al][ga] R_b[ga][ga'] conj(M^{s'}[al'][ga'])``.  The state need not be normalised; the result is
        Hermitian to rounding.  1 <= width <= min(n, 6), 0 <= start <= n - width."""
        n = len(self.tensors)
        for name, v in (("start", start), ("width", width)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"{name} must be an int, got {v!r}")
        a, w = int(start), int(width)
        if not 1 <= w <= min(n, 6):
            raise ValueError(f"width must be in 1 .. min(n, 6) = {min(n, 6)}, got {width!r}")
        if not 0 <= a <= n - w:
            raise ValueError(f"start must be in 0 .. n - width = {n - w}, got {start!r}")
        ts = [np.asarray(t, dtype=np.complex128) for t in self.tensors]
        L = np.ones((1, 1), dtype=np.complex128)  # L[ket][bra]
        for k in range(a):
            L = np.einsum("ab,asc,bsd->cd", L, ts[k], ts[k].conj(), optimize=True)
        R = np.ones((1, 1), dtype=np.complex128)  # R[ket][bra]
        for k in range(n - 1, a + w - 1, -1):
            R = np.einsum("asc,cd,bsd->ab", ts[k], R, ts[k].conj(), optimize=True)
        M = ts[a]  # M[al][s][ga], s growing to the right: the new site is the least significant bit
        for k in range(a + 1, a + w):
            M = np.tensordot(M, ts[k], axes=(2, 0)).reshape(M.shape[0], -1, ts[k].shape[2])
        rho = np.einsum("ab,asc,cd,btd->st", L, M, R, M.conj(), optimize=True)
        return rho / np.trace(rho).real

    def operator_expectation(self, table, codes) -> np.ndarray:
        """Expectation values ``<psi| O_0 (x) ... (x) O_{n-1} |psi> / <psi|psi>`` of strings of single-site operators on the host,
        complex128 of shape (m,) (``()`` for a single row of codes): the numpy mirror of ``Context.operator_expectations``.
        ``table`` is (n_ops, 2, 2) with ``table[c - 1][s'][s] = <s'|O_c|s>``, ``codes`` (n,) or (m, n) of codes 0 .. n_ops (0 =
        identity), as ``engine.operator_strings`` makes them.  A plain environment loop: every L_k and R_k in the X[ket][bra]
        orientation, then per string ``E = L_a``, ``E <- sum_{s,s'} O[s'][s] A^s^T E conj(A^s')`` over the support [a, b] and
        ``sum E R_{b+1} / <psi|psi>``.  An all-identity row is exactly 1 + 0j.  The state need not be normalised; a state of norm 0
        raises ``ValueError``."""
        from .engine import _operator_table

        n = len(self.tensors)
        t = _operator_table(table)
        c = np.asarray(codes)
        single = c.ndim == 1
        if single:
            c = c[None, :]
        if c.dtype.kind not in "iu" or c.ndim != 2 or c.shape[1] != n or c.shape[0] < 1:
            raise ValueError(f"codes must be an integer array of shape ({n},) or (m >= 1, {n}); got shape {np.shape(codes)}, dtype {c.dtype}")
        if c.min() < 0 or c.max() > len(t):
            raise ValueError(f"codes holds a value outside 0 .. n_ops = {len(t)} ({int(c.min() if c.min() < 0 else c.max())})")
        ts = [np.asarray(a, dtype=np.complex128) for a in self.tensors]
        L, R = [None] * (n + 1), [None] * (n + 1)  # [ket][bra] at bond k
        L[0] = np.ones((1, 1), dtype=np.complex128)
        R[n] = np.ones((1, 1), dtype=np.complex128)
        for k in range(n):
            L[k + 1] = np.einsum("ab,asc,bsd->cd", L[k], ts[k], ts[k].conj(), optimize=True)
        for k in range(n - 1, -1, -1):
            R[k] = np.einsum("asc,cd,bsd->ab", ts[k], R[k + 1], ts[k].conj(), optimize=True)
        norm = float(L[n][0, 0].real)
        if norm == 0.0:
            raise ValueError("operator_expectation: the state has norm 0")
        out = np.ones(c.shape[0], dtype=np.complex128)
        for m, row in enumerate(c):
            supp = np.flatnonzero(row)
            if supp.size == 0:
                continue
            E = L[supp[0]]
            for k in range(supp[0], supp[-1] + 1):
                if row[k]:
                    E = np.einsum("ab,asc,ts,btd->cd", E, ts[k], t[row[k] - 1], ts[k].conj(), optimize=True)
                else:
                    E = np.einsum("ab,asc,bsd->cd", E, ts[k], ts[k].conj(), optimize=True)
            out[m] = (E * R[supp[-1] + 1]).sum() / norm
        return out[0] if single else out

    def mpo_expectation(self, mpo) -> complex:
        """``<psi| H |psi> / <psi|psi>`` of an ``engine.Mpo`` on the host, complex: the numpy mirror of
        ``Context.mpo_expectations`` and the oracle for sizes a dense matrix cannot reach.  A plain environment loop in the
        X[ket][bra] orientation with one plane per MPO bond state: ``E[0] = L_a``, ``E'[v] = sum_{u,s,s'} W_k[u][v][s'][s] A^s^T
        E[u] conj(A^s')`` over the support [a, b] (the hull of the sites whose tensor is not exactly the 1 x 1 identity), then
        ``sum E[0] R_{b+1} / <psi|psi>``.  An MPO without a support is exactly 1 + 0j.  The state need not be normalised; a state
        of norm 0 raises ``ValueError``."""
        from .engine import Mpo

        n = len(self.tensors)
        if not isinstance(mpo, Mpo):
            raise ValueError(f"mpo_expectation takes an engine.Mpo, got {type(mpo).__name__}")
        if mpo.n_sites != n:
            raise ValueError(f"the Mpo has {mpo.n_sites} sites, the state has {n}")
        ts = [np.asarray(a, dtype=np.complex128) for a in self.tensors]
        L, R = [None] * (n + 1), [None] * (n + 1)  # [ket][bra] at bond k
        L[0] = np.ones((1, 1), dtype=np.complex128)
        R[n] = np.ones((1, 1), dtype=np.complex128)
        for k in range(n):
            L[k + 1] = np.einsum("ab,asc,bsd->cd", L[k], ts[k], ts[k].conj(), optimize=True)
        for k in range(n - 1, -1, -1):
            R[k] = np.einsum("asc,cd,bsd->ab", ts[k], R[k + 1], ts[k].conj(), optimize=True)
        norm = float(L[n][0, 0].real)
        if norm == 0.0:
            raise ValueError("mpo_expectation: the state has norm 0")
        eye = np.eye(2, dtype=np.complex128).reshape(1, 1, 2, 2)
        supp = [k for k, w in enumerate(mpo.tensors) if w.shape != eye.shape or not np.array_equal(w, eye)]
        if not supp:
            return 1.0 + 0.0j
        E = L[supp[0]][None]  # [u][ket][bra]
        for k in range(supp[0], supp[-1] + 1):
            T = np.tensordot(E, ts[k], axes=(1, 0))                             # [u][b][s][c]
            T = np.tensordot(mpo.tensors[k], T, axes=([0, 3], [0, 2]))          # [v][t][b][c]
            E = np.tensordot(T, ts[k].conj(), axes=([1, 2], [1, 0]))            # [v][c][d]
        return complex((E[0] * R[supp[-1] + 1]).sum() / norm)

    def apply_mpo(self, mpo) -> "MPS":
        """``O|psi>`` of an ``engine.Mpo`` as a new ``MPS`` on the host: the numpy mirror of ``Context.apply_mpo`` and its oracle.
        Site k of the product is ``B_k[(u, a)][s'][(v, b)] = sum_s W_k[u][v][s'][s] A_k[a][s][b]`` with row ``u chi_k + a`` and
        column ``v chi_{k+1} + b`` (u and v major), so its bonds are ``w_k chi_k``.  Nothing is truncated or normalised and the
        gauge is general; the state itself is untouched."""
        from .engine import Mpo

        n = len(self.tensors)
        if not isinstance(mpo, Mpo):
            raise ValueError(f"apply_mpo takes an engine.Mpo, got {type(mpo).__name__}")
        if mpo.n_sites != n:
            raise ValueError(f"the Mpo has {mpo.n_sites} sites, the state has {n}")
        out = []
        for W, A in zip(mpo.tensors, self.tensors):
            A = np.asarray(A, dtype=np.complex128)
            B = np.einsum("uvts,asb->uatvb", W, A)
            out.append(np.ascontiguousarray(B.reshape(W.shape[0] * A.shape[0], 2, W.shape[1] * A.shape[2])))
        return MPS(out)

    def marginal(self, bits, bases) -> np.ndarray:
        """Probabilities of partial outcomes on the host, float64 of shape (n_strings,): the numpy mirror of ``Context.marginals``.
        ``bits`` is (n_strings, n) of 0 / 1 (bit 0 = eigenvalue +1), ``bases`` (n_strings, n) or one shared row of codes 0..3: 0 =
        not measured (traced out; the bit there is ignored), 1, 2, 3 = X, Y, Z.  The real part of ``operator_expectation`` on
        ``engine.marginal_strings(bits, bases, n)``; not clipped, so a probability of exactly 0 may come out as rounding noise of
        either sign.  A row with no measured qubit is exactly 1.0."""
        from .engine import marginal_strings

        table, codes = marginal_strings(bits, bases, len(self.tensors))
        return np.ascontiguousarray(self.operator_expectation(table, codes).real)

    def sample(self, shots: int, bases=None, seed: int = 0, state_index: int = 0, logp: bool = False, margin: bool = False):
        """Measurement shots of the state on the host, the numpy mirror of ``Context.sample``: ``bits`` uint8 (shots, n), bit 0 =
        eigenvalue +1 of the Pauli (``bases``, anything ``engine.bases_table`` takes; codes 1..3 = X, Y, Z) the qubit was measured
        in.  The right environments ``R_k`` come from the loop of the other mirrors; then per shot, v = [1], for k = 0 .. n-1:
        ``W_t = v A_k[:, t, :]``, rotated into the basis (Z: as it is; X: (W_0 +- W_1)/sqrt2; Y: (W_0 -+ i W_1)/sqrt2),
        ``p_o = max(0, Re W'_o R_{k+1} W'_o^H)``, ``bit = 1 if p_1 > 0 and u (p_0 + p_1) >= p_0`` with ``u =
        engine.sample_uniform(seed, state_index, shot, k)``, ``v = W'_bit / sqrt(p_bit)``.  ``logp=True`` adds the log of the exact
        probability of each drawn string, ``margin=True`` the smallest ``|u tot - p_0| / tot`` over all draws (how far the nearest
        draw sat from its threshold): the result is ``bits`` or the tuple ``(bits[, logp][, margin])``.  A state of norm 0 raises
        ``ValueError``."""
        from .engine import bases_table, sample_uniform

        n = len(self.tensors)
        if isinstance(shots, bool) or not isinstance(shots, (int, np.integer)) or shots < 1:
            raise ValueError(f"shots must be an int >= 1 (got {shots!r})")
        S = int(shots)
        B = bases_table(bases, S, n)
        if B.min() < 1 or B.max() > 3:
            raise ValueError("bases holds a code outside 1..3 = X, Y, Z")
        ts = [np.asarray(t, dtype=np.complex128) for t in self.tensors]
        R = [None] * (n + 1)  # R[ket][bra] at bond k
        R[n] = np.ones((1, 1), dtype=np.complex128)
        for k in range(n - 1, 0, -1):
            R[k] = np.einsum("asc,cd,bsd->ab", ts[k], R[k + 1], ts[k].conj(), optimize=True)
        u = sample_uniform(seed, state_index, np.arange(S)[:, None], np.arange(n)[None, :])
        h = 0.70710678118654752440
        v = np.ones((S, 1), dtype=np.complex128)
        bits = np.zeros((S, n), dtype=np.uint8)
        lp = np.zeros(S, dtype=np.float64)
        worst = np.inf
        for k in range(n):
            W = np.einsum("rb,btc->rtc", v, ts[k])
            W0, W1 = W[:, 0], W[:, 1]
            code = B[:, k][:, None]
            A0 = np.where(code == 1, (W0 + W1) * h, np.where(code == 2, (W0 - 1j * W1) * h, W0))
            A1 = np.where(code == 1, (W0 - W1) * h, np.where(code == 2, (W0 + 1j * W1) * h, W1))
            p0 = np.maximum(0.0, np.einsum("rb,ba,ra->r", A0, R[k + 1], A0.conj()).real)
            p1 = np.maximum(0.0, np.einsum("rb,ba,ra->r", A1, R[k + 1], A1.conj()).real)
            tot = p0 + p1
            if not (np.all(tot > 0.0) and np.all(np.isfinite(tot))):
                raise ValueError(f"sample: the outcome probabilities of site {k} sum to 0 or are not finite (a state of norm 0?)")
            bit = (p1 > 0.0) & (u[:, k] * tot >= p0)
            worst = min(worst, float(np.min(np.abs(u[:, k] * tot - p0) / tot)))
            pb = np.where(bit, p1, p0)
            lp += np.log(pb / tot)
            v = np.where(bit[:, None], A1, A0) / np.sqrt(pb)[:, None]
            bits[:, k] = bit
        out = (bits,) + ((lp,) if logp else ()) + ((worst,) if margin else ())
        return out if len(out) > 1 else bits

    def amplitude(self, bits, bases=None, scaled: bool = False, logp: bool = False, dtype=np.complex128):
        """Amplitudes ``<b| U_bases |psi>`` of given outcome strings on the host, the numpy mirror of ``Context.amplitudes``:
        ``bits`` is (n,) or (S, n) of 0 / 1 (bit 0 = eigenvalue +1), ``bases`` anything ``engine.bases_table`` takes (codes 1..3 =
        X, Y, Z; ``None``: all Z).  Per string, v = [1], E = 0, for k = 0 .. n-1: ``W_t = v A_k[:, t, :]``, rotated into the basis
        (Z: as it is; X: (W_0 +- W_1)/sqrt2; Y: (W_0 -+ i W_1)/sqrt2), ``u = W'_bit``, ``m = max_a max(|Re u[a]|, |Im u[a]|)``;
        ``m > 0``: ``m = f 2^e`` with 0.5 <= f < 1 (frexp), ``v = u 2^-e`` (exact), ``E += e``; ``m == 0``: ``v = 0``, ``E = 0``.  The
        amplitude is ``v_n[0] 2^E``: complex128 of shape (S,) (``()`` for a single string), which may underflow to 0;
        ``scaled=True`` returns ``(mant, expo int32)`` instead, the larger component of ``mant`` in [0.5, 1) or ``mant`` exactly 0
        with ``expo`` 0.  ``logp=True`` appends ``2 (log |mant| + expo log 2) - log <psi|psi>`` (-inf for a zero amplitude; a
        state of norm 0 raises ``ValueError``).  ``dtype=np.clongdouble`` runs the same loop in extended precision (what the tests
        measure the float64 loop against)."""
        from .engine import bases_table

        n = len(self.tensors)
        b = np.asarray(bits)
        single = b.ndim == 1
        if single:
            b = b[None, :]
        if b.dtype.kind not in "iub" or b.ndim != 2 or b.shape[1] != n or b.shape[0] < 1:
            raise ValueError(f"bits must be an integer array of shape ({n},) or (n_strings >= 1, {n}); got shape {np.shape(bits)}, dtype {b.dtype}")
        if b.min() < 0 or b.max() > 1:
            raise ValueError("bits holds a value that is not 0 or 1")
        S = b.shape[0]
        B = bases_table(bases, S, n)
        if B.min() < 1 or B.max() > 3:
            raise ValueError("bases holds a code outside 1..3 = X, Y, Z")
        cdt = np.dtype(dtype)
        rdt = np.empty(0, dtype=cdt).real.dtype
        ts = [np.asarray(t, dtype=cdt) for t in self.tensors]
        h = rdt.type(1) / np.sqrt(rdt.type(2)) if cdt != np.complex128 else rdt.type(0.70710678118654752440)
        v = np.ones((S, 1), dtype=cdt)
        E = np.zeros(S, dtype=np.int64)
        for k in range(n):
            W = np.einsum("rb,btc->rtc", v, ts[k])
            W0, W1 = W[:, 0], W[:, 1]
            code = B[:, k][:, None]
            A0 = np.where(code == 1, (W0 + W1) * h, np.where(code == 2, (W0 - 1j * W1) * h, W0))
            A1 = np.where(code == 1, (W0 - W1) * h, np.where(code == 2, (W0 + 1j * W1) * h, W1))
            u = np.where(b[:, k][:, None] == 1, A1, A0)
            m = np.maximum(np.abs(u.real), np.abs(u.imag)).max(axis=1)
            e = np.where((m > 0) & np.isfinite(m), np.frexp(m)[1], 0).astype(np.int64)
            v = (np.ldexp(u.real, -e[:, None]) + 1j * np.ldexp(u.imag, -e[:, None])).astype(cdt)
            E = np.where(m == 0, 0, E + e)  # a zero amplitude is (0, 0) with E = 0, whatever came before
        mant, expo = v[:, 0], E.astype(np.int32)
        out = (mant, expo) if scaled else ((np.ldexp(mant.real, expo) + 1j * np.ldexp(mant.imag, expo)).astype(cdt),)
        if logp:
            R = np.ones((1, 1), dtype=np.complex128)
            for t in reversed(self.tensors):
                t = np.asarray(t, dtype=np.complex128)
                R = np.einsum("asc,cd,bsd->ab", t, R, t.conj(), optimize=True)
            norm = float(R[0, 0].real)
            if not (norm > 0.0 and np.isfinite(norm)):
                raise ValueError("amplitude: the state has norm 0 (or a norm that is not finite): logp is not defined")
            a = np.abs(mant).astype(np.float64)
            with np.errstate(divide="ignore"):
                out += (np.where(a == 0.0, -np.inf, 2.0 * (np.log(a) + expo * np.log(2.0)) - np.log(norm)),)
        if single:
            out = tuple(o[0] for o in out)
        return out if len(out) > 1 else out[0]

    def vdot(self, other: "MPS") -> complex:
        """<self|other> through the HIP engine (single pair; the Gram path is batch-first)."""
        from .engine import default_context

        if len(other) != len(self):
            raise RuntimeError("the two MPS must have the same number of sites")
        ctx = default_context()
        with ctx.upload([self]) as xs, ctx.upload([other]) as ys:
            return complex(ctx.overlaps(xs, ys)[0, 0])


def random_mps(n_sites: int, bond_dims, rng) -> MPS:
    """Random normalised MPS with a prescribed bond profile ``bond_dims[0..n]`` (pure-kernel
    benchmark inputs): complex Gaussian tensors, right-orthonormalised by QR."""
    chi = [int(c) for c in bond_dims]
    assert len(chi) == n_sites + 1 and chi[0] == 1 and chi[-1] == 1
    ts = [
        (rng.standard_normal((chi[k], 2, chi[k + 1])) + 1j * rng.standard_normal((chi[k], 2, chi[k + 1])))
        for k in range(n_sites)
    ]
    for k in range(n_sites - 1, 0, -1):
        l, _, r = ts[k].shape
        q, rr = np.linalg.qr(ts[k].reshape(l, 2 * r).T)  # (2r, l) = q (2r, m) rr (m, l)
        m = q.shape[1]
        if m != l:
            raise ValueError(f"bond {k}: dimension {l} exceeds what its neighbours allow ({m})")
        ts[k] = q.T.reshape(l, 2, r)
        ts[k - 1] = np.tensordot(ts[k - 1], rr.T, axes=(2, 0))
    ts[0] = ts[0] / np.linalg.norm(ts[0])
    return MPS(ts)


def _kept(s: np.ndarray, discard_budget: float, zero: float) -> tuple[int, float]:
    """How many leading singular values survive, and the kept fraction of the weight.

    Values <= ``zero`` (absolute; the state is normalised) are dropped first, then the
    smallest values are dropped while their summed weight stays within
    ``discard_budget`` of the total -- both sums accumulated from the small end.
    """
    w = s * s
    total = float(w.sum())
    keep = int(np.count_nonzero(s > zero))
    keep = max(keep, 1)
    tail = np.cumsum(w[:keep][::-1])  # tail[m-1] = weight of the m smallest candidates
    drop = int(np.searchsorted(tail, discard_budget * total, side="right"))
    keep = max(keep - drop, 1)
    return keep, float(w[:keep].sum()) / total


def seed_state(state: MPS, value_of_zero: float = 1e-16):
    """A given state made ready for the builders: ``(MPS, norm)``, the numpy mirror of the sweep path of ``Context.seed``.  The
    state may be in any gauge and of any norm: ``MPS.compress(max_discard=0)`` takes it to left-canonical form with the centre on
    the last site (a bond whose rank is below its dimension shrinks to its rank), then the last site is divided by its Frobenius
    norm ``norm`` = sqrt(<psi|psi>).  The result has norm 1, centre n - 1 and carries the sweep's fidelity.  ``ValueError`` for a
    state of norm 0 or with an entry that is not finite."""
    if not isinstance(state, MPS):
        raise ValueError(f"seed_state needs an MPS, got {type(state).__name__}")
    if not all(np.isfinite(t).all() for t in state.tensors):
        raise ValueError("seed_state: the state has an entry that is not finite")
    out, _ = state.compress(None, 0.0, value_of_zero)
    last = out.tensors[-1]
    norm = float(np.sqrt(float((last.real * last.real + last.imag * last.imag).sum())))
    if not (norm > 0.0 and np.isfinite(norm)):
        raise ValueError(f"seed_state: the state has norm {norm!r}")
    out.tensors[-1] = last / norm
    return out, norm


def _initial_state(circuit, initial, initial_centre, value_of_zero):
    """The state a host build starts from: ``None`` (|0...0>), or ``(MPS, centre)`` -- ``initial`` as it stands with its centre on
    ``initial_centre``, or, without one, seeded by ``seed_state``.  ``ValueError`` by name for what cannot be built from."""
    if initial is None:
        if initial_centre is not None:
            raise ValueError("initial_centre goes with an initial state")
        return None
    if not isinstance(initial, MPS):
        raise ValueError(f"initial must be an MPS, got {type(initial).__name__}")
    n = circuit.n_qubits
    if len(initial) != n:
        raise ValueError(f"the initial state has {len(initial)} sites, the circuit {n} qubits")
    if initial_centre is None:
        return seed_state(initial, value_of_zero)[0], n - 1
    if isinstance(initial_centre, bool) or not isinstance(initial_centre, (int, np.integer)) or not 0 <= int(initial_centre) < n:
        raise ValueError(f"initial_centre must be a site in 0 .. {n - 1} (got {initial_centre!r})")
    if not all(np.isfinite(t).all() for t in initial.tensors) or not (np.isfinite(initial.fidelity) and np.isfinite(initial.logw)):
        raise ValueError("the initial state has an entry that is not finite")
    return initial, int(initial_centre)


_NATIVE = None  # ctypes handle of libqkbuilder.so, False once loading has failed


def _native_builder():
    """The native host builder (csrc/qk_builder.cpp), or None: it needs libqkbuilder.so (built by
    ``__graft_entry__.build()``) and the OpenBLAS that scipy ships (for zgesdd / zgeqrf / zungqr / zgemm)."""
    global _NATIVE
    if _NATIVE is None:
        import ctypes as C
        import glob
        import os

        _NATIVE = False
        try:
            import scipy

            here = os.path.dirname(os.path.abspath(__file__))
            blas = sorted(glob.glob(os.path.join(os.path.dirname(scipy.__file__), "..", "scipy.libs", "libscipy_openblas*.so")))
            lib = C.CDLL(os.path.join(here, "libqkbuilder.so"))
            lib.qkb_last_error.restype = C.c_char_p
            lib.qkb_init.argtypes = [C.c_char_p]
            lib.qkb_simulate_program.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            _program.check_sizes(lib, {"qkb_program_size": _program.QkProgram, "qkb_run_size": _program.QkbRun, "qkb_result_size": _program.QkbResult})
            lib.qkb_free.argtypes = [C.c_void_p]
            if blas and lib.qkb_init(os.path.realpath(blas[0]).encode()) == 0:
                _NATIVE = lib
        except OSError:
            _NATIVE = False
    return _NATIVE or None


def _condition_rows(circuit, op):
    """The condition rows of ``circuit`` as the native entries take them: (cond_gate int32, cond_mask uint32 or None)."""
    cg = np.ascontiguousarray(circuit.cond_gate, dtype=np.int32)
    cm = None if circuit.cond_mask is None else np.ascontiguousarray(np.asarray(circuit.cond_mask).astype(np.uint32))
    if cg.shape != op.shape or (cm is not None and cm.shape != op.shape):
        raise ValueError(f"a program with conditions needs a cond_gate and a cond_mask per gate, got shapes {cg.shape}, {None if cm is None else cm.shape}")
    return cg, cm


def simulate_native(circuit: BoundCircuit, truncation_fidelity: float = 1.0 - 1e-16, value_of_zero: float = 1e-16, max_bond: int | None = None, seed=0, state_index=0,
                    trajectory=0, first_gate=0, margin=False, initial=None, initial_centre=None):
    """``simulate`` through the native builder (``qkb_simulate_program``): same algorithm and LAPACK routines, no interpreter in the
    gate loop.  The circuit's tables and condition rows go over as they are -- the native builder validates them -- with the
    trajectory arguments and ``margin`` as in ``simulate``.  With ``initial`` (and ``initial_centre``, as in ``simulate``) the state
    is seeded here, the native builder only loads it."""
    import ctypes as C

    lib = _native_builder()
    if lib is None:
        raise RuntimeError("native MPS builder unavailable (libqkbuilder.so or scipy's OpenBLAS not found)")
    n = circuit.n_qubits
    op = np.ascontiguousarray(circuit.op, dtype=np.int8)
    tables = {}
    if circuit.mats is not None and circuit.mat is not None:  # the matrix table of codes 8 and 9
        mats = np.ascontiguousarray(circuit.mats, dtype=np.complex128)
        mat = np.ascontiguousarray(circuit.mat, dtype=np.int32)
        if mats.ndim != 3 or mats.shape[1:] != (4, 4) or mat.shape != op.shape:
            raise ValueError(f"the matrix table must be [n_mats][4][4] with one index per gate, got shapes {mats.shape} and {mat.shape}")
        tables.update(mats=mats, mat=mat)
    seed, state_index, trajectory, first_gate = _trajectory_ids(seed, state_index, trajectory, first_gate)
    start = _initial_state(circuit, initial, initial_centre, value_of_zero)
    n_kgates = 0
    if circuit.channel is not None:  # the channel tables of codes 10 and 11
        for d, names in ((2, ("kraus", "n_kraus")), (4, ("kraus2", "n_kraus2"))):
            k, nk = (getattr(circuit, a) for a in names)
            if k is None or nk is None:
                continue
            k, nk = np.ascontiguousarray(k, dtype=np.complex128), np.ascontiguousarray(nk, dtype=np.int32)
            if k.ndim != 4 or k.shape[1:] != (d * d, d, d) or nk.shape != k.shape[:1]:
                raise ValueError(f"the channel table must be [n_channels][{d * d}][{d}][{d}] with a count per channel, got shapes {k.shape}, {nk.shape}")
            tables.update(zip(names, (k, nk)))
        if "kraus" in tables or "kraus2" in tables:
            channel = np.ascontiguousarray(circuit.channel, dtype=np.int32)
            branch = np.full(op.shape, -1, dtype=np.int32) if circuit.branch is None else np.ascontiguousarray(circuit.branch, dtype=np.int32)
            if channel.shape != op.shape or branch.shape != op.shape:
                raise ValueError(f"a program with a channel table needs a channel and a branch per gate, got shapes {channel.shape}, {branch.shape}")
            tables.update(channel=channel, branch=branch)
            n_kgates = int(np.count_nonzero((op == OP_K1) | (op == OP_K2)))
    if circuit.cond_gate is not None:  # without a channel table the native builder refuses the rows
        tables.update(zip(("cond_gate", "cond_mask"), _condition_rows(circuit, op)))
    prog = _program.fill_program(1, n, op, np.ascontiguousarray(circuit.q0, dtype=np.int32), np.ascontiguousarray(circuit.alpha, dtype=np.float64), seed=seed,
                                 state_index=np.array([state_index], dtype=np.uint32), trajectory=np.array([trajectory], dtype=np.uint32), first_gate=first_gate, **tables)
    run = _program.sized(_program.QkbRun, max_bond=int(max_bond or 0), trunc_budget=max(0.0, 1.0 - float(truncation_fidelity)), value_of_zero=float(value_of_zero))
    if start is not None:
        init_dims = np.ascontiguousarray(start[0].bond_dims(), dtype=np.int32)
        init_flat = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.complex128).ravel() for t in start[0].tensors]))
        run.init_dims, run.init_tensors, run.init_centre, run.init_fidelity, run.init_logw = init_dims.ctypes.data, init_flat.ctypes.data, start[1], start[0].fidelity, start[0].logw
    dims = np.zeros(n + 1, dtype=np.int32)
    branches = np.full(max(1, n_kgates), -1, dtype=np.int8)
    res = _program.sized(_program.QkbResult, dims=dims.ctypes.data, branches=branches.ctypes.data)
    rc = lib.qkb_simulate_program(C.byref(prog), C.byref(run), C.byref(res))
    if rc in (-7, -8, -9):  # an op code outside the program's vocabulary; a bad matrix or channel gate; an impossible outcome of a channel
        raise ValueError(f"native MPS builder: {lib.qkb_last_error().decode()}")
    if rc != 0:
        raise RuntimeError(f"native MPS builder failed: {lib.qkb_last_error().decode()}")
    try:
        flat = np.ctypeslib.as_array(C.cast(res.tensors, C.POINTER(C.c_double)), shape=(2 * res.n_complex,)).view(np.complex128).copy()
    finally:
        lib.qkb_free(res.tensors)
    tensors, pos = [], 0
    for k in range(n):
        sz = int(dims[k]) * 2 * int(dims[k + 1])
        tensors.append(flat[pos : pos + sz].reshape(int(dims[k]), 2, int(dims[k + 1])))
        pos += sz
    out = MPS(tensors, res.fidelity, res.logw, branches[:n_kgates])
    return (out, float(res.margin)) if margin else out


def simulate(circuit: BoundCircuit, truncation_fidelity: float = 1.0 - 1e-16, value_of_zero: float = 1e-16, max_bond: int | None = None, checkpoints=None, seed=0,
             state_index=0, trajectory=0, first_gate=0, margin=False, initial=None, initial_centre=None):
    """MPS of circuit|0...0>, "MPSxGate" style: one SVD per two-qubit gate (ref :221).  ``max_bond``: at most that many singular
    values survive a gate -- the ``chi`` of pytket-cutensornet's ``Config`` (ref :141-144 is where it would go); the weight it
    costs goes into ``fidelity`` like any other truncation.

    ``checkpoints=[c_0, ..., n_gates]`` (gate counts: strictly increasing, in 1 .. n_gates, the last one n_gates) is the host mirror
    of ``Context.build_mps_scan``: the result is a ``list[MPS]``, entry j a copy of the state after c_j gates with its fidelity so
    far, in the mixed-canonical gauge the run left it in; the last entry is ``simulate(circuit)`` of the numpy loop bit for bit.  It
    always runs the numpy loop (the native builder keeps no snapshots), whatever QK_NATIVE_BUILDER says.

    A circuit with Kraus channels (op code 10) is run as one quantum trajectory: the branch of a drawn channel gate i comes from
    ``engine.channel_uniform(seed, first_gate + i, trajectory, state_index)``, so a (state, trajectory) pair names its draws whatever
    else is built with it, and a run resumed at gate ``first_gate`` draws what the uninterrupted one draws.  The result carries
    ``logw`` and ``branches``; ``margin=True`` returns ``(result, margin)`` (see ``_simulate``).

    ``initial`` (an ``MPS`` of ``n_qubits`` sites) replaces |0...0>: the circuit is applied to that state.  With
    ``initial_centre=None`` the state may be in any gauge and of any norm and is seeded by ``seed_state`` first (canonical, norm 1,
    centre n - 1, the sweep's fidelity); with ``initial_centre=k`` it is taken as it stands, canonical with its centre on site k, and
    the run begins with ``initial.fidelity`` and ``initial.logw`` -- the host form of resuming from ``scan.states(j)``, whose centre
    ``scan.info(j)`` reports.  Conditions may not reach behind the initial state.  ``initial=None`` is the code path without it.

    The matrices are small (tens to a few hundred rows): a multi-threaded BLAS spends its time waking
    threads (measured 24 s instead of 0.9 s per 60-qubit state on 8 cores), so the LAPACK calls run
    single-threaded here; parallelism is across states (``builder_pool.build_states``)."""
    if checkpoints is not None:
        checkpoints = check_checkpoints(checkpoints, circuit.n_gates)
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:  # pragma: no cover - optional dependency
        return _simulate(circuit, truncation_fidelity, value_of_zero, max_bond, checkpoints, seed, state_index, trajectory, first_gate, margin, initial, initial_centre)
    with threadpool_limits(limits=1):
        if checkpoints is not None:
            return _simulate(circuit, truncation_fidelity, value_of_zero, max_bond, checkpoints, seed, state_index, trajectory, first_gate, margin, initial, initial_centre)
        if _use_native():
            return simulate_native(circuit, truncation_fidelity, value_of_zero, max_bond, seed, state_index, trajectory, first_gate, margin, initial, initial_centre)
        return _simulate(circuit, truncation_fidelity, value_of_zero, max_bond, None, seed, state_index, trajectory, first_gate, margin, initial, initial_centre)


def simulate_many(circuits, truncation_fidelity: float = 1.0 - 1e-16, value_of_zero: float = 1e-16, workers: int | None = None, progress=None, max_bond: int | None = None,
                  initial=None):
    """``simulate`` for a list of circuits on several host cores **without forking** (safe once the GPU is initialised).
    The first circuit is built in this process and sizes the job: long jobs go to one worker *process* per core
    (``builder_worker.py`` over pipes: 10.8x on 16 cores for cfg4-shaped circuits, where threads in one process reach 2x
    because concurrent LAPACK calls contend inside OpenBLAS), medium ones to a thread pool (the native builder is a ctypes
    call that releases the GIL), short ones stay serial.  QK_BUILDER_POOL=procs|threads|serial overrides the choice.
    ``initial`` (one ``MPS`` for all circuits, or a list with one per circuit) starts them from given states (``simulate``); such
    a job stays in this process (threads or serial).  Returns (list[MPS], seconds per circuit)."""
    import time

    circuits = list(circuits)
    reject_channels(circuits, "simulate_many")
    if not circuits:
        return [], []
    if workers is None:
        from .builder_pool import default_workers

        workers = default_workers()
    workers = max(1, min(int(workers), len(circuits) - 1))
    if initial is not None:
        inits = [initial] * len(circuits) if isinstance(initial, MPS) else list(initial)
        if len(inits) != len(circuits):
            raise ValueError(f"simulate_many: {len(inits)} initial states for {len(circuits)} circuits")
        circuits = list(zip(circuits, inits))  # a job is (circuit, initial state)

    def one(c):
        t0 = time.perf_counter()
        m = simulate(c, truncation_fidelity, value_of_zero, max_bond) if initial is None else simulate(c[0], truncation_fidelity, value_of_zero, max_bond, initial=c[1])
        if progress is not None:
            progress()
        return m, time.perf_counter() - t0

    first, t_first = one(circuits[0])
    rest = circuits[1:]
    estimate = t_first * len(rest)  # serial seconds still to do
    mode = os.environ.get("QK_BUILDER_POOL", "auto")
    if mode == "auto":
        mode = "procs" if estimate / max(1, workers) > 2.0 else ("threads" if estimate > 0.5 else "serial")
    if not rest or workers <= 1:
        mode = "serial"
    if mode == "procs" and initial is not None:
        mode = "threads"
    if mode == "threads" and not _use_native():
        mode = "serial"
    if mode == "procs":
        out, secs = _simulate_many_procs(rest, truncation_fidelity, value_of_zero, workers, progress, max_bond)
    elif mode == "threads":
        from concurrent.futures import ThreadPoolExecutor

        def one_native(c):  # simulate() would enter / leave the BLAS thread limit per call, racing across threads
            t0 = time.perf_counter()
            m = simulate_native(c, truncation_fidelity, value_of_zero, max_bond) if initial is None else simulate_native(c[0], truncation_fidelity, value_of_zero, max_bond, initial=c[1])
            if progress is not None:
                progress()
            return m, time.perf_counter() - t0

        try:
            from threadpoolctl import threadpool_limits
        except ImportError:  # pragma: no cover - optional dependency
            threadpool_limits = None
        limit = threadpool_limits(limits=1) if threadpool_limits else None
        try:
            with ThreadPoolExecutor(max_workers=workers) as pool:
                res = list(pool.map(one_native, rest))
        finally:
            if limit is not None:
                limit.restore_original_limits()
        out, secs = [m for m, _ in res], [dt for _, dt in res]
    else:
        res = [one(c) for c in rest]
        out, secs = [m for m, _ in res], [dt for _, dt in res]
    return [first] + out, [t_first] + secs


def _simulate_many_procs(circuits, truncation_fidelity, value_of_zero, workers, progress, max_bond=None):
    """One interpreter per core (builder_worker.py) fed over pipes by one thread each; tasks are handed out one at a time,
    so uneven circuits balance themselves."""
    import pickle
    import subprocess
    import sys
    import threading

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"import sys; sys.path.insert(0, {root!r}); import qml_cutensornet_amd.builder_worker as w; w.main()"
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, "-c", code], stdin=subprocess.PIPE, stdout=subprocess.PIPE, env=env) for _ in range(workers)]
    results, errors = [None] * len(circuits), []
    lock, nxt = threading.Lock(), [0]

    def feed(pr):
        try:
            while True:
                with lock:
                    i = nxt[0]
                    nxt[0] += 1
                if i >= len(circuits) or errors:
                    break
                pickle.dump((i, circuits[i], truncation_fidelity, value_of_zero, max_bond), pr.stdin, protocol=4)
                pr.stdin.flush()
                idx, tensors, fid, dt, err = pickle.load(pr.stdout)
                if err is not None:
                    raise RuntimeError(f"builder worker failed on circuit {idx}: {err}")
                results[idx] = (MPS(tensors, fid), dt)
                if progress is not None:
                    progress()
        except Exception as exc:  # noqa: BLE001 - collected and re-raised in the caller's thread
            errors.append(exc)
        finally:
            try:
                pr.stdin.close()
            except OSError:
                pass

    threads = [threading.Thread(target=feed, args=(pr,), daemon=True) for pr in procs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for pr in procs:
        try:
            pr.wait(timeout=30)
        except subprocess.TimeoutExpired:
            pr.kill()
    if errors:
        raise RuntimeError(f"host builder pool: {errors[0]}")
    return [r[0] for r in results], [r[1] for r in results]


def _use_native() -> bool:
    """QK_NATIVE_BUILDER=0 forces the numpy/scipy loop; otherwise the native builder is used when it loads."""
    import os

    return os.environ.get("QK_NATIVE_BUILDER", "1") != "0" and _native_builder() is not None


def _trajectory_ids(seed, state_index, trajectory, first_gate):
    from .engine import _seed_key

    _seed_key(seed)
    for name, v in (("state_index", state_index), ("trajectory", trajectory), ("first_gate", first_gate)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < 1 << 32:
            raise ValueError(f"{name} must be an int in 0 .. 2^32 - 1 (got {v!r})")
    return int(seed), int(state_index), int(trajectory), int(first_gate)


def _simulate(circuit: BoundCircuit, truncation_fidelity: float, value_of_zero: float, max_bond: int | None = None, checkpoints=None, seed=0, state_index=0, trajectory=0,
              first_gate=0, margin=False, initial=None, initial_centre=None):
    """The numpy loop.  With ``checkpoints`` (validated gate counts) the return value is the list of snapshots: copies, the run itself
    is the one without them.  A circuit with a matrix table (``circuit.mat``, ``circuit.mats``) may hold op codes 8 and 9, a 2x2 on q0
    and a 4x4 on (q0, q0+1); ``ValueError`` for a table entry that is not unitary, an index outside the table or a gate outside
    the register.

    A circuit with a two-qubit channel table (``kraus2``, ``n_kraus2``) may hold op code 11, a two-qubit Kraus channel on (q, q+1):
    the centre is brought into the pair and ``theta = A_q A_{q+1}`` formed as for any two-qubit gate; ``N = sum |theta|^2``, ``p_k = sum
    |K_k theta|^2``, the branch as for code 10 below (same uniform); ``theta <- (K_b / sqrt(p_b)) theta``, then the SVD, truncation,
    fidelity product and centre placement of a two-qubit gate -- the bond may shrink or be cut --, and ``logw += log(p_b / N)``.
    ``branches`` counts the gates of both codes in program order.

    A circuit with a channel table (``channel``, ``branch``, ``kraus``, ``n_kraus``) may hold op code 10, a one-qubit Kraus channel:
    the centre is brought onto site q exactly, ``N = sum |A_q|^2``, ``p_k = sum |K_k A_q|^2``, ``tot = p_0 + .. + p_{m-1}``; the branch b
    is ``branch[i]`` or, drawn, the first k with ``p_k > 0`` and ``u tot < p_0 + .. + p_k`` (none: the last k with ``p_k > 0``) for
    ``u = engine.channel_uniform(seed, first_gate + i, trajectory, state_index)``; ``A_q <- (K_b / sqrt(p_b)) A_q`` and ``logw +=
    log(p_b / N)``.  The result carries ``logw`` and ``branches``; with ``margin`` the return value is ``(result, margin)``, the
    smallest ``|u tot - cum| / tot`` over the thresholds of all draws (inf without one).  ``ValueError`` naming the state and the gate
    for an impossible outcome (``p_b`` 0 or not finite, ``tot`` 0 in a draw).

    Classical control (``cond_gate``, ``cond_mask``; a channel table is needed): gate i with ``cond_gate[i] = g >= 0`` runs when the
    branch b recorded for gate g is ``>= 0`` and bit b of ``cond_mask[i]`` is set; else it is skipped -- no centre move, no theta, no
    SVD, no draw, nothing added to ``logw`` or the margin -- and a skipped channel gate records branch -2.  A skipped gate is a done
    gate for the checkpoints, and the look-ahead ``two_q_pos`` counts it: where a two-qubit gate leaves the centre is a function of
    the op codes alone."""
    n = circuit.n_qubits
    chan = check_channel_gates(circuit.op, circuit.q0, n, circuit.channel, circuit.branch, circuit.kraus, circuit.n_kraus, circuit.kraus2, circuit.n_kraus2)
    mat, mats = check_matrix_gates(circuit.op, circuit.mat, circuit.mats, with_channels=chan is not None and chan[2] is not None,
                                   with_channels2=chan is not None and chan[4] is not None)  # (None, None): no table, codes 8 and 9 are unknown
    seed, state_index, trajectory, first_gate = _trajectory_ids(seed, state_index, trajectory, first_gate)
    cond = check_condition_gates(circuit.op, chan, circuit.cond_gate, circuit.cond_mask)  # None: no gate is conditional
    logw, branches, worst = 0.0, [], np.inf
    taken = {}  # the branch every channel gate took, by position (-2: skipped): what conditions read

    def take_branch(i, forced, p):
        """The branch of channel gate i with probabilities p (the forced one, or drawn), and the running margin."""
        from .engine import channel_uniform

        m, low = len(p), worst
        tot = 0.0
        for k in range(m):
            tot += p[k]
        where = f"state {state_index}, gate {first_gate + i}"
        if forced >= 0:
            b = forced
        else:
            if not (tot > 0.0 and np.isfinite(tot)):
                raise ValueError(f"simulate: {where}: the branch probabilities of the channel sum to {tot!r}")
            u = float(channel_uniform(seed, first_gate + i, trajectory, state_index))
            b, cum, last = -1, 0.0, -1
            for k in range(m):
                cum += p[k]
                if k < m - 1:
                    low = min(low, abs(u * tot - cum) / tot)
                if p[k] > 0.0:
                    last = k
                    if b < 0 and u * tot < cum:
                        b = k
            if b < 0:
                b = last
        if not (p[b] > 0.0 and np.isfinite(p[b])):
            raise ValueError(f"simulate: {where}: branch {b} of the channel has probability {p[b]!r} (an impossible outcome was post-selected?)")
        return b, low

    for i, (o, q) in enumerate(zip(circuit.op.tolist(), circuit.q0.tolist())):
        if not 0 <= q < n - (1 if is_two_qubit(o) else 0):
            raise ValueError(f"gate {i} on a qubit outside the register of {n}")
    budget = max(0.0, 1.0 - float(truncation_fidelity))
    A = []
    for _ in range(n):
        t = np.zeros((1, 2, 1), dtype=np.complex128)
        t[0, 0, 0] = 1.0
        A.append(t)
    ops = circuit.op.tolist()
    qs = circuit.q0.tolist()
    alphas = circuit.alpha.tolist()
    two_q_pos = [q for o, q in zip(ops, qs) if is_two_qubit(o)]
    fidelity = 1.0
    centre = 0  # sites < centre are left-orthonormal, sites > centre right-orthonormal
    start = _initial_state(circuit, initial, initial_centre, value_of_zero)
    if start is not None:  # the run goes on from a given state (``simulate``): its sites, centre, fidelity and log-weight
        A = [np.array(t, dtype=np.complex128) for t in start[0].tensors]
        centre, fidelity, logw = start[1], start[0].fidelity, start[0].logw
    g2 = 0  # running index into two_q_pos
    snaps, marks = [], set(checkpoints or ())

    for i, (o, q, a) in enumerate(zip(ops, qs, alphas)):
        if i in marks:  # i gates done
            snaps.append(MPS([t.copy() for t in A], fidelity, logw, branches))
        if cond is not None and cond[0][i] >= 0:  # a gate whose condition is false does nothing at all; it is a done gate all the same
            b = taken[int(cond[0][i])]
            if b < 0 or not (int(cond[1][i]) >> b) & 1:
                if o in (OP_K1, OP_K2):
                    taken[i] = -2
                    branches.append(-2)
                g2 += is_two_qubit(o)  # the look-ahead is a function of the op codes alone
                continue
        if o == OP_H:
            t = A[q]
            A[q] = np.stack((t[:, 0] + t[:, 1], t[:, 0] - t[:, 1]), axis=1) * _SQRT_HALF
            continue
        if o == OP_RZ:
            th = 0.5 * np.pi * a
            ph = complex(np.cos(th), np.sin(th))
            t = A[q].copy()
            t[:, 0] *= ph.conjugate()
            t[:, 1] *= ph
            A[q] = t
            continue
        if o == OP_M1:  # a 2x2 from the table: new[p] = sum_s M[p][s] old[s]
            m = mats[mat[i]]
            t = A[q]
            A[q] = np.stack((m[0, 0] * t[:, 0] + m[0, 1] * t[:, 1], m[1, 0] * t[:, 0] + m[1, 1] * t[:, 1]), axis=1)
            continue
        if not is_two_qubit(o) and o != OP_K1:  # Rx: [[c, -i s], [-i s, c]];  Ry: [[c, -s], [s, c]]
            th = 0.5 * np.pi * a
            c, sn = np.cos(th), np.sin(th)
            m01, m10 = (-1j * sn, -1j * sn) if o == OP_RX else (-sn, sn)
            t = A[q]
            A[q] = np.stack((c * t[:, 0] + m01 * t[:, 1], m10 * t[:, 0] + c * t[:, 1]), axis=1)
            continue

        # ---- two-qubit gate on (q, q+1): bring the orthogonality centre onto the pair; a channel on q: onto the site
        lo, hi = (q, q) if o == OP_K1 else (q, q + 1)
        while centre < lo:
            l, _, r = A[centre].shape
            qq, rr = _qr(A[centre].reshape(l * 2, r), mode="economic", check_finite=False)
            A[centre] = qq.reshape(l, 2, -1)
            A[centre + 1] = np.tensordot(rr, A[centre + 1], axes=(1, 0))
            centre += 1
        while centre > hi:
            l, _, r = A[centre].shape
            qq, rr = _qr(A[centre].reshape(l, 2 * r).T, mode="economic", check_finite=False)
            A[centre] = qq.T.reshape(-1, 2, r)
            A[centre - 1] = np.tensordot(A[centre - 1], rr.T, axes=(2, 0))
            centre -= 1

        if o == OP_K1:  # the channel step: the centre stays on q, the bonds do not change
            c, forced = int(chan[0][i]), int(chan[1][i])
            m = int(chan[3][c])
            K = chan[2][c]
            t = A[q]
            t0, t1 = t[:, 0], t[:, 1]
            N = float((t.real * t.real + t.imag * t.imag).sum())
            p = []
            for k in range(m):
                y0, y1 = K[k, 0, 0] * t0 + K[k, 0, 1] * t1, K[k, 1, 0] * t0 + K[k, 1, 1] * t1
                p.append(float((y0.real * y0.real + y0.imag * y0.imag + y1.real * y1.real + y1.imag * y1.imag).sum()))
            b, worst = take_branch(i, forced, p)
            Kb = K[b] / np.sqrt(p[b])
            A[q] = np.stack((Kb[0, 0] * t0 + Kb[0, 1] * t1, Kb[1, 0] * t0 + Kb[1, 1] * t1), axis=1)
            logw += float(np.log(p[b] / N))
            branches.append(b)
            taken[i] = b
            continue

        l = A[q].shape[0]
        r = A[q + 1].shape[2]
        theta = np.tensordot(A[q], A[q + 1], axes=(2, 0))  # [l, p, p', r]
        if o == OP_SWAP:
            theta = theta.transpose(0, 2, 1, 3)
        elif o == OP_YY:  # cos(th) 1 - i sin(th) Y(x)Y
            th = 0.5 * np.pi * a
            theta = np.cos(th) * theta + 1j * np.sin(th) * _YY_SIGN * theta[:, ::-1, ::-1, :]
        elif o == OP_ZZ:  # diag(e^-i th, e^i th, e^i th, e^-i th)
            th = 0.5 * np.pi * a
            ph = np.exp(1j * th)
            theta = theta * np.array([[ph.conjugate(), ph], [ph, ph.conjugate()]])[None, :, :, None]
        elif o == OP_M2:  # a 4x4 from the table: new[(p,p')] = sum M[(p,p')][(s,s')] old[(s,s')]
            theta = np.einsum("pqst,lstr->lpqr", mats[mat[i]].reshape(2, 2, 2, 2), theta)
        elif o == OP_K2:  # a two-qubit Kraus channel: code 10's branch logic on theta, then the SVD of any two-qubit gate
            c, forced = int(chan[0][i]), int(chan[1][i])
            K = chan[4][c, : int(chan[5][c])].reshape(-1, 2, 2, 2, 2)
            N = float((theta.real * theta.real + theta.imag * theta.imag).sum())
            p = [0.0] * K.shape[0]
            for k in range(K.shape[0]) if forced < 0 else [forced]:  # a forced branch needs p_b only
                y = np.einsum("pqst,lstr->lpqr", K[k], theta)
                p[k] = float((y.real * y.real + y.imag * y.imag).sum())
            b, worst = take_branch(i, forced, p)
            theta = np.einsum("pqst,lstr->lpqr", K[b] / np.sqrt(p[b]), theta)
            logw += float(np.log(p[b] / N))
            branches.append(b)
            taken[i] = b
        else:  # XXPhase: cos(th) 1 - i sin(th) X(x)X
            th = 0.5 * np.pi * a
            theta = np.cos(th) * theta - 1j * np.sin(th) * theta[:, ::-1, ::-1, :]
        u, s, vh = _svd(
            np.ascontiguousarray(theta).reshape(l * 2, 2 * r),
            full_matrices=False,
            lapack_driver="gesdd",
            check_finite=False,
            overwrite_a=True,
        )
        keep, frac = _kept(s, budget, value_of_zero)
        if max_bond and keep > max_bond:  # the chi cap
            keep = int(max_bond)
            frac = float((s[:keep] ** 2).sum() / (s ** 2).sum())
        fidelity *= frac
        s = s[:keep]
        s = s / np.sqrt(float((s * s).sum()))
        g2 += 1
        nxt = two_q_pos[g2] if g2 < len(two_q_pos) else q
        if nxt >= q + 1 or (nxt == q and True):
            # leave the centre on q+1 (also right for a repeat on the same pair)
            A[q] = u[:, :keep].reshape(l, 2, keep)
            A[q + 1] = (s[:, None] * vh[:keep]).reshape(keep, 2, r)
            centre = q + 1
        else:
            A[q] = (u[:, :keep] * s[None, :]).reshape(l, 2, keep)
            A[q + 1] = vh[:keep].reshape(keep, 2, r)
            centre = q
    out = snaps + [MPS(A, fidelity, logw, branches)] if checkpoints is not None else MPS(A, fidelity, logw, branches)
    return (out, float(worst)) if margin else out
