#!/usr/bin/env python3
"""Time the projected quantum kernel against the fidelity Gram on one MI355X, in one process: the config's states built by the
device builder, then (each after a warm-up) ctx.gram(xs), ctx.local_paulis(xs), ctx.projected_gram(F) and the two-qubit form,
ctx.local_pair_paulis(xs) and ctx.projected_pair_gram(T).  Prints one JSON line with the five times, the algorithmic flops of the
two local sweeps and their achieved TFLOP/s.  ``--pair-distance D`` (D > 1) adds the pairs up to distance D:
ctx.local_pair_paulis(xs, max_dist=D) and ctx.projected_pair_gram(T, max_dist=D), their times, flops and median entry.
``--strings N`` (N sparse Pauli strings: weight 1..4 inside a window of 6 sites, seeded) or ``--strings-file F`` (one string over
IXYZ per line) adds ctx.pauli_expectations(xs, strings) and ctx.feature_gram(V): pauli_strings_ms, n_strings, sum_support.
``--entanglement`` adds ctx.bond_purities(xs) and ctx.bond_spectra(xs): bond_purities_ms, bond_spectra_ms, and what a bond cap
would discard, ``cap_cost`` summed over the bonds of a state at chi = 16, 32, 64, 128 (the mean and the largest over the states).
``--compress CHI`` adds ctx.compress(xs, max_bond=CHI) and the Gram of the compressed set: compress_ms, compressed_gram_ms,
compressed_max_bond, min_fidelity and max_abs_dK = max |K(compressed) - K|.
``--block-widths 10,20,30,60`` adds the block kernels of the first w qubits: ctx.block_values_host on the symmetric plan of all
pairs and ctx.block_self(xs, widths): block_values_ms, block_self_ms, n_widths, block_over_gram and, per width, the median
off-diagonal entry of the "normalized" kernel.
``--shots S`` adds ctx.sample(xs, S, bases=engine.random_bases(S, n, 0)): sample_ms, shots, sample_flops (the two GEMMs of every
site for every shot, from the true bonds) and sample_tflops, and the median off-diagonal entry of the kernel estimated from the shots.
``--block-shots U,M`` (with ``--block-widths``, widths <= 32) adds the block overlaps at finite shots: ctx.sample in
engine.setting_bases(U, M, n, 0), then ctx.shot_block_sums_host on the pairs of the same symmetric plan (the call uploads the
outcome bytes, packs them and sums): shot_block_ms (the median; shot_block_ms_min and _max give the spread over the repetitions),
shot_block_terms = pairs U M^2 n_widths, shot_block_terms_per_s, shot_block_over_block against block_values_ms of the same run, and per
width the median off-diagonal estimate next to the exact one.
``--shadow-shots T`` (with ``--shots``) adds the shot-pair histograms of the classical-shadow kernel: ctx.sample in
engine.random_bases(T, n, 0), then ctx.shadow_hist_host on the pairs of the run's symmetric plan (the call uploads the outcome bytes,
packs them, counts and downloads the histograms), after a warm-up: shadow_hist_ms (the median; shadow_hist_ms_min and _max give the
spread over the repetitions), shadow_shot_pairs = pairs T^2, shadow_shot_pairs_per_s, shadow_over_sample against sample_ms of the same
run, and the median off-diagonal entry of the shadow kernel at gamma = tau = 1.
``--shot-strings W`` (with ``--shots``, 1 <= W <= 6) adds the window RDMs estimated from those shots: ctx.estimate_window_rdms(bits,
bases, W) on all n - W + 1 windows (the call uploads the outcome bytes, packs them, tests every shot against the (n - W + 1) 4^W
strings and rebuilds the RDMs), after a warm-up: shot_strings_ms (the median; shot_strings_ms_min and _max give the spread over the
repetitions), n_shot_strings, shot_string_tests = states x shots x strings, shot_string_tests_per_s, shot_strings_over_sample against
sample_ms of the same run, and shot_strings_mirror_ms: the numpy mirror engine.estimate_window_rdms on the first 8 states of the same
input (shot_strings_mirror_states; one run, not scaled up), with shot_strings_mirror_equal = the two agree bit for bit there.
``--window W`` (1 <= W <= 6) adds the k-qubit projected kernel: ctx.window_rdms(xs, W) on all n - W + 1 windows and
ctx.projected_window_gram(rho), each after a warm-up: window_rdms_ms (the median; window_rdms_ms_min and _max give the spread over the
repetitions), window_width, n_windows, window_flops and window_tflops, projected_window_gram_ms, window_over_pair against
local_pair_paulis_ms of the same run, and median_offdiag_pqk_window.  window_flops, from the true bonds at 8 flops per complex
multiply-add: the environment pass (the GEMMs of the one-qubit sweep, ``local_sweep_flops``) and, for every window [a, b = a + W) of
every state, the steps j = 0 .. W-1 at site c = b-1-j -- two products (t = 0, 1) of chi_c x 2^j chi_b over chi_c+1 for the seed R_b
and, from j = 1 on, for the seed 1 -- then H (chi_a x 2^W chi_b over chi_a) and the closing sum (2^W (2^W + 1) / 2 entries of chi_a
chi_b terms).
``--amplitudes S`` adds the amplitudes of given strings: S shots per state drawn with ctx.sample in engine.random_bases(S, n, 0)
(timed like ``--shots``), then ctx.amplitudes(xs, bits, bases, per_state=True, logp=True) on them, after a warm-up: amplitudes_ms (the
median; amplitudes_ms_min and _max give the spread over the repetitions), amp_strings = S, amp_flops and amp_tflops, amp_sample_ms
and amp_over_sample = amplitudes_ms / amp_sample_ms of the same run, and max_abs_dlogp_amp_sample = max |logp_amplitudes -
logp_sample|.  amp_flops, from the true bonds at 8 flops per complex multiply-add: per state, site and string the row of W = V (A^0 |
A^1) (1 x 2 chi_k+1 over chi_k), i.e. S sum 8 (2 chi_k+1 chi_k), plus the environment pass that gives <psi|psi> for logp
(``local_sweep_flops``).
``--marginals N`` (with ``--strings`` or ``--strings-file``) adds the marginals of partial outcomes: N projector strings on the
supports of the tool's Pauli strings (string j takes the support of Pauli string j mod n_strings), random bases X, Y, Z and random bits
on the measured qubits (seeded), through ctx.marginals(xs, bits, bases), after a warm-up: marginals_ms (the median; marginals_ms_min
and _max give the spread over the repetitions), n_marginals and sum_support (of the marginal strings: marginals_sum_support), and
opstr_over_pauli = the time of the Pauli table sent through ctx.operator_expectations on the tool's own strings (opstr_pauli_ms, with
_min and _max) over pauli_strings_ms of the same run, with max_abs_d_opstr_pauli = max |value - pauli_expectations|.
usage: python tools/pqk_time.py --config cfg3|cfg4|cfg5 [--gamma G] [--reps N] [--pair-distance D] [--strings N | --strings-file F] [--entanglement] [--compress CHI]
                                [--block-widths W1,W2,... [--block-shots U,M]] [--shots S [--shadow-shots T] [--shot-strings W]] [--window W] [--amplitudes S] [--marginals N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import qml_cutensornet_amd as Q  # noqa: E402
from qml_cutensornet_amd import engine  # noqa: E402
from qml_cutensornet_amd.data import synthetic_features  # noqa: E402


def local_sweep_flops(dims):
    """Algorithmic flops of the local sweep from the true bonds (8 per complex multiply-add).  Per site, l = chi_k, r = chi_k+1:
    the T-shaped GEMM of each direction (forward: l x 2r over l; reversed: r x 2l over r) and three of the second shape (the
    reversed chain's environment update, l x l over 2r, and the two W_s, r x 2r over l)."""
    d = np.asarray(dims, dtype=np.float64)
    l, r = d[:, :-1], d[:, 1:]
    return float((8 * (l * 2 * r * l + r * 2 * l * r) + 8 * (l * l * 2 * r + 2 * r * 2 * r * l)).sum())


def pair_sweep_flops(dims):
    """The pair sweep adds, for every site but the first (l = chi_k, r = chi_k+1), a second T-shaped GEMM on the reversed image
    (r x 2l over r) and the two V_t (l x 2l over r)."""
    d = np.asarray(dims, dtype=np.float64)
    l, r = d[:, 1:-1], d[:, 2:]
    return local_sweep_flops(dims) + float((8 * (r * 2 * l * r) + 8 * (2 * l * 2 * l * r)).sum())


def dist_sweep_flops(dims, D):
    """Pairs up to distance D add, at every site k = 1 .. n-2 (l = chi_k, r = chi_k+1) and for each of the min(k, D - 1) live
    origins, four T-shaped GEMMs (l x 2r over l) and four closing ones (r x r over 2l)."""
    d = np.asarray(dims, dtype=np.float64)
    n = d.shape[1] - 1
    total = pair_sweep_flops(dims)
    for k in range(1, n - 1):
        l, r = d[:, k], d[:, k + 1]
        total += float((min(k, D - 1) * 4 * 8 * (l * 2 * r * l + r * r * 2 * l)).sum())
    return total


def sample_flops(dims, shots):
    """Algorithmic flops of sampling ``shots`` shots of every state from the true bonds (8 per complex multiply-add).  Per site and
    shot, l = chi_k, r = chi_k+1: the row of W = V (A^0 | A^1) (1 x 2r over l) and the two rows of Q = [W'_0 ; W'_1] R (2 x r over r)."""
    d = np.asarray(dims, dtype=np.float64)
    l, r = d[:, :-1], d[:, 1:]
    return float(shots * (8 * (2 * r * l) + 8 * (2 * r * r)).sum())


def amplitude_flops(dims, strings):
    """Algorithmic flops of ``amplitudes(..., logp=True)`` on ``strings`` strings per state from the true bonds (8 per complex
    multiply-add).  Per site and string, l = chi_k, r = chi_k+1: the row of W = V (A^0 | A^1) (1 x 2r over l); and once per state
    the environment pass that gives <psi|psi> (``local_sweep_flops``)."""
    d = np.asarray(dims, dtype=np.float64)
    l, r = d[:, :-1], d[:, 1:]
    return float(strings * (8 * (2 * r * l)).sum()) + local_sweep_flops(dims)


def window_flops(dims, w):
    """Algorithmic flops of ``window_rdms(xs, w)`` on all windows, from the true bonds (the formula of the module docstring)."""
    d = np.asarray(dims, dtype=np.float64)
    n = d.shape[1] - 1
    total = local_sweep_flops(dims)
    D = 2.0**w
    for a in range(n - w + 1):
        b = a + w
        for j in range(w):
            c = b - 1 - j
            total += float(((2 if j else 1) * 2 * 8 * d[:, c] * (2.0**j) * d[:, b] * d[:, c + 1]).sum())
        total += float((8 * d[:, a] * D * d[:, b] * d[:, a] + 8 * (D * (D + 1) / 2) * d[:, a] * d[:, b]).sum())
    return total


def sparse_strings(n, count, seed=0):
    """``count`` sparse strings on n qubits: weight 1..4 inside a window of 6 sites at a random position, random codes X, Y, Z."""
    rng = np.random.default_rng(seed)
    S = np.zeros((count, n), dtype=np.uint8)
    w = min(6, n)
    for row in S:
        sites = rng.integers(0, n - w + 1) + rng.choice(w, size=rng.integers(1, min(4, w) + 1), replace=False)
        row[sites] = rng.integers(1, 4, size=len(sites))
    return S


def timed(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, 1e3 * float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4", choices=("cfg3", "cfg4", "cfg5"))
    ap.add_argument("--gamma", type=float, default=None, help="default 1.0 (0.1 for cfg5)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pair-distance", type=int, default=1, help="also time the pairs up to this distance (default 1: neighbours only)")
    ap.add_argument("--strings", type=int, default=0, help="also time pauli_expectations on this many sparse Pauli strings")
    ap.add_argument("--strings-file", default=None, help="also time pauli_expectations on the strings of this file (one per line over IXYZ)")
    ap.add_argument("--entanglement", action="store_true", help="also time bond_purities and bond_spectra and print the cost of a bond cap")
    ap.add_argument("--compress", type=int, default=0, metavar="CHI", help="also time compress(max_bond=CHI) and the Gram of the compressed set")
    ap.add_argument("--block-widths", default=None, metavar="W1,W2,...", help="also time the block kernels of the first w qubits for these widths")
    ap.add_argument("--block-shots", default=None, metavar="U,M", help="with --block-widths: also time the block overlaps estimated from U settings of M shots")
    ap.add_argument("--shots", type=int, default=0, metavar="S", help="also time sample() with S shots per state in random bases")
    ap.add_argument("--shadow-shots", type=int, default=0, metavar="T", help="with --shots: also time the shadow kernel's shot-pair histograms from T shots per state")
    ap.add_argument("--shot-strings", type=int, default=0, metavar="W", help="with --shots: also time estimate_window_rdms at width W on the sampled shots")
    ap.add_argument("--window", type=int, default=0, metavar="W", help="also time window_rdms on all windows of W qubits and projected_window_gram")
    ap.add_argument("--amplitudes", type=int, default=0, metavar="S", help="also time amplitudes() with logp on S shots per state drawn with sample()")
    ap.add_argument("--marginals", type=int, default=0, metavar="N", help="with --strings: also time marginals() on N projector strings on the supports of those strings")
    ap.add_argument("--mpo", default=None, choices=("heisenberg", "exponential"), help="also time mpo_expectations on this MPO (heisenberg: also its term list through operator_expectations)")
    ap.add_argument("--apply", default=None, choices=("parity", "heisenberg_step", "gate"),
                    help="also time apply_mpo with this MPO (parity: the even projector; heisenberg_step: 1 - 0.05i H; gate: a Haar 4 x 4 on qubits (0, n - 1)) and the compress that follows")
    ap.add_argument("--apply-max-gib", type=float, default=64.0, help="with --apply: the largest product image; wider states are capped first")
    args = ap.parse_args()
    if args.block_shots and not args.block_widths:
        ap.error("--block-shots needs --block-widths")
    if args.shadow_shots and args.shots <= 0:
        ap.error("--shadow-shots needs --shots (shadow_over_sample compares with its sample_ms)")
    if args.marginals and not (args.strings > 0 or args.strings_file):
        ap.error("--marginals needs --strings or --strings-file (it measures on their supports, and opstr_over_pauli compares with their pauli_strings_ms)")
    if args.shot_strings and args.shots <= 0:
        ap.error("--shot-strings needs --shots (it estimates from those shots, and shot_strings_over_sample compares with their sample_ms)")
    if args.shot_strings and not 1 <= args.shot_strings <= engine.WINDOW_MAX_WIDTH:
        ap.error(f"--shot-strings takes a width in 1 .. {engine.WINDOW_MAX_WIDTH}")
    gamma = args.gamma if args.gamma is not None else (0.1 if args.config == "cfg5" else 1.0)
    n, reps, d, npts = bench.CONFIGS[args.config]
    X = synthetic_features(npts, n, 5)
    ans = Q.KernelStateAnsatz(n, reps, gamma, Q.entanglement_graph(n, d))
    ctx = engine.Context(0)
    t0 = time.perf_counter()
    xs, states, info = ctx.build_share([ans.circuit_for_data(x) for x in X], 1.0 - 1e-16, max_bond=320)
    if xs is None:
        raise SystemExit(f"{len(info['dropped'])} states outgrew the device builder's bond cap")
    build_s = time.perf_counter() - t0
    ctx.trim()
    K, gram_ms = timed(lambda: ctx.gram(xs), args.reps)
    F, local_ms = timed(lambda: ctx.local_paulis(xs), args.reps)
    KP, pgram_ms = timed(lambda: ctx.projected_gram(F), args.reps)
    T, pair_ms = timed(lambda: ctx.local_pair_paulis(xs), args.reps)
    KP2, pgram2_ms = timed(lambda: ctx.projected_pair_gram(T), args.reps)
    flops, flops2 = local_sweep_flops(info["dims"]), pair_sweep_flops(info["dims"])
    off = ~np.eye(npts, dtype=bool)
    dist = {}
    if args.pair_distance > 1:
        D = args.pair_distance
        TD, dist_ms = timed(lambda: ctx.local_pair_paulis(xs, max_dist=D), args.reps)
        KPD, pgramd_ms = timed(lambda: ctx.projected_pair_gram(TD, max_dist=D), args.reps)
        flopsd = dist_sweep_flops(info["dims"], D)
        dist = {
            "pair_distance": D, "n_pairs": int(TD.shape[1]), "local_pair_dist_ms": round(dist_ms, 3),
            "projected_pair_dist_gram_ms": round(pgramd_ms, 3), "dist_over_pair": round(dist_ms / pair_ms, 4),
            "dist_flops": flopsd, "dist_tflops": round(flopsd / (dist_ms * 1e-3) / 1e12, 3),
            "dist_block_one_is_pair_bits": bool(np.array_equal(TD[:, : n - 1], T)),
            "median_offdiag_pqk2_dist": float(np.median(KPD[off])),
        }
    if args.strings > 0 or args.strings_file:
        if args.strings_file:
            with open(args.strings_file) as fh:
                S = engine.pauli_strings(n, [line.strip() for line in fh if line.strip()])
        else:
            S = sparse_strings(n, args.strings)
        V, strings_ms = timed(lambda: ctx.pauli_expectations(xs, S), args.reps)
        KO, fgram_ms = timed(lambda: ctx.feature_gram(V), args.reps)
        support = [int(np.flatnonzero(c)[-1] - np.flatnonzero(c)[0] + 1) if c.any() else 0 for c in S]
        dist.update({
            "n_strings": int(len(S)), "sum_support": int(sum(support)), "pauli_strings_ms": round(strings_ms, 3),
            "feature_gram_ms": round(fgram_ms, 3), "strings_over_local": round(strings_ms / local_ms, 4),
            "median_offdiag_feature_K": float(np.median(KO[off])),
        })
    if args.marginals > 0:
        rng = np.random.default_rng(1)
        mask = S[np.arange(args.marginals) % len(S)] != 0
        m_bases = np.where(mask, rng.integers(1, 4, size=mask.shape), 0).astype(np.uint8)
        m_bits = np.where(mask, rng.integers(0, 2, size=mask.shape), 0).astype(np.uint8)

        def spread(fn):
            fn()  # warm-up
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                out = fn()
                ts.append(1e3 * (time.perf_counter() - t0))
            return out, ts

        Pm, ts_m = spread(lambda: ctx.marginals(xs, m_bits, m_bases))
        pauli_table = np.stack([engine.LOCAL_OPS[name] for name in "XYZ"])
        Vo, ts_o = spread(lambda: ctx.operator_expectations(xs, S, ops=pauli_table))
        m_support = [int(np.flatnonzero(c)[-1] - np.flatnonzero(c)[0] + 1) if c.any() else 0 for c in mask]
        dist.update({
            "n_marginals": int(args.marginals), "marginals_sum_support": int(sum(m_support)), "marginals_reps": args.reps,
            "marginals_ms": round(float(np.median(ts_m)), 3), "marginals_ms_min": round(min(ts_m), 3), "marginals_ms_max": round(max(ts_m), 3),
            "opstr_pauli_ms": round(float(np.median(ts_o)), 3), "opstr_pauli_ms_min": round(min(ts_o), 3), "opstr_pauli_ms_max": round(max(ts_o), 3),
            "opstr_over_pauli": round(float(np.median(ts_o)) / strings_ms, 4), "max_abs_d_opstr_pauli": float(np.abs(Vo - V).max()),
            "min_marginal": float(Pm.min()), "max_marginal": float(Pm.max()),
        })
    if args.entanglement:
        P, pur_ms = timed(lambda: ctx.bond_purities(xs), args.reps)
        S, spec_ms = timed(lambda: ctx.bond_spectra(xs), args.reps)
        s1 = engine.bond_entropies(S)
        costs = {chi: engine.cap_cost(S, chi).sum(axis=1) for chi in (16, 32, 64, 128)}
        dist.update({
            "bond_purities_ms": round(pur_ms, 3), "bond_spectra_ms": round(spec_ms, 3), "spectra_values": int(S.shape[2]),
            "purity_minus_sum_sq": float(np.abs(P - (S * S).sum(-1)).max()), "max_entropy_S1": float(s1.max()),
            "median_max_entropy_S1": float(np.median(s1.max(axis=1))),
            "median_weights_above_1e-3": float(np.median(engine.schmidt_rank(S, 1e-3).max(axis=1))),
            "cap_cost": {str(chi): {"mean": float(c.mean()), "max": float(c.max())} for chi, c in costs.items()},
        })
    if args.compress > 0:
        def squeeze():
            cs, cinfo = ctx.compress(xs, max_bond=args.compress, info=True)
            cs.close()
            return cinfo

        cinfo, compress_ms = timed(squeeze, args.reps)
        with ctx.compress(xs, max_bond=args.compress) as cs:
            KC, cgram_ms = timed(lambda: ctx.gram(cs), args.reps)
        dist.update({
            "compress_chi": int(args.compress), "compress_ms": round(compress_ms, 3), "compressed_gram_ms": round(cgram_ms, 3),
            "compressed_max_bond": int(cinfo["bond_dims"].max()), "min_fidelity": float(cinfo["fidelity"].min()),
            "max_abs_dK": float(np.abs(KC - K).max()),
        })
    if args.block_widths:
        widths = [int(w) for w in args.block_widths.split(",")]
        plan = engine.Plan(xs.dims, orient=False)
        vals, block_ms = timed(lambda: ctx.block_values_host(xs, None, plan, widths), args.reps)
        Sw, self_ms = timed(lambda: ctx.block_self(xs, widths), args.reps)
        pairs = plan.pairs()
        plan.close()
        offd = pairs[:, 0] != pairs[:, 1]
        norm = vals / np.sqrt(Sw[:, pairs[:, 0]] * Sw[:, pairs[:, 1]])
        dist.update({
            "block_widths": widths, "n_widths": len(widths), "block_values_ms": round(block_ms, 3), "block_self_ms": round(self_ms, 3),
            "block_over_gram": round(block_ms / gram_ms, 4),
            "median_offdiag_block_normalized": {str(w): float(np.median(norm[wi][offd])) for wi, w in enumerate(widths)},
        })
        if args.block_shots:
            U, M = (int(v) for v in args.block_shots.split(","))
            bits = ctx.sample(xs, U * M, bases=engine.setting_bases(U, M, n, 0), seed=0)
            ctx.shot_block_sums_host(bits, None, U, pairs, widths)  # warm-up
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                sums = ctx.shot_block_sums_host(bits, None, U, pairs, widths)
                ts.append(1e3 * (time.perf_counter() - t0))
            shot_ms = float(np.median(ts))
            est = engine.shot_block_estimate(sums, None, U, M, ~offd)[0]
            terms = len(pairs) * U * M * M * len(widths)
            dist.update({
                "block_shots": [U, M], "shot_block_reps": args.reps, "shot_block_ms": round(shot_ms, 3), "shot_block_ms_min": round(min(ts), 3),
                "shot_block_ms_max": round(max(ts), 3), "shot_block_terms": terms, "shot_block_terms_per_s": round(terms / (shot_ms * 1e-3), 1),
                "shot_block_over_block": round(shot_ms / block_ms, 4),
                "median_offdiag_block_shots": {str(w): float(np.median(est[wi][offd])) for wi, w in enumerate(widths)},
                "median_offdiag_block_exact": {str(w): float(np.median(vals[wi][offd])) for wi, w in enumerate(widths)},
            })
    if args.shots > 0:
        bases = engine.random_bases(args.shots, n, 0)
        bits, sample_ms = timed(lambda: ctx.sample(xs, args.shots, bases=bases, seed=0), args.reps)
        sflops = sample_flops(info["dims"], args.shots)
        KS = ctx.projected_gram(engine.estimate_paulis(bits, bases)[0])
        dist.update({
            "shots": int(args.shots), "sample_ms": round(sample_ms, 3), "sample_flops": sflops,
            "sample_tflops": round(sflops / (sample_ms * 1e-3) / 1e12, 3), "sample_over_local": round(sample_ms / local_ms, 4),
            "median_offdiag_pqk_shots": float(np.median(KS[off])),
        })
    if args.shadow_shots > 0:
        T_sh = args.shadow_shots
        sh_bases = engine.random_bases(T_sh, n, 0)
        sh_bits = ctx.sample(xs, T_sh, bases=sh_bases, seed=0)
        plan = engine.Plan(xs.dims, orient=False)
        sh_pairs = plan.pairs()
        plan.close()
        ctx.shadow_hist_host(sh_bits, sh_bases, pairs=sh_pairs)  # warm-up
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            H = ctx.shadow_hist_host(sh_bits, sh_bases, pairs=sh_pairs)
            ts.append(1e3 * (time.perf_counter() - t0))
        shadow_ms = float(np.median(ts))
        shot_pairs = len(sh_pairs) * T_sh * T_sh
        KSH = engine.shadow_kernel(H, n)
        dist.update({
            "shadow_shots": T_sh, "shadow_reps": args.reps, "shadow_pairs": int(len(sh_pairs)), "shadow_hist_ms": round(shadow_ms, 3),
            "shadow_hist_ms_min": round(min(ts), 3), "shadow_hist_ms_max": round(max(ts), 3), "shadow_shot_pairs": shot_pairs,
            "shadow_shot_pairs_per_s": round(shot_pairs / (shadow_ms * 1e-3), 1), "shadow_over_sample": round(shadow_ms / dist["sample_ms"], 4),
            "median_offdiag_shadow": float(np.median(KSH[sh_pairs[:, 0] != sh_pairs[:, 1]])),
        })
    if args.shot_strings > 0:
        W_ss = args.shot_strings
        n_ss = (n - W_ss + 1) * 4**W_ss
        ctx.estimate_window_rdms(bits, bases, W_ss)  # warm-up
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            rho_hat, _ = ctx.estimate_window_rdms(bits, bases, W_ss)
            ts.append(1e3 * (time.perf_counter() - t0))
        ss_ms = float(np.median(ts))
        t0 = time.perf_counter()
        mirror_rho, _ = engine.estimate_window_rdms(bits[:8], bases, W_ss)
        mirror_ms = 1e3 * (time.perf_counter() - t0)
        tests = npts * args.shots * n_ss
        KSS = ctx.projected_window_gram(rho_hat)
        dist.update({
            "shot_strings_width": W_ss, "n_shot_strings": n_ss, "shot_strings_reps": args.reps, "shot_strings_ms": round(ss_ms, 3),
            "shot_strings_ms_min": round(min(ts), 3), "shot_strings_ms_max": round(max(ts), 3), "shot_string_tests": tests,
            "shot_string_tests_per_s": round(tests / (ss_ms * 1e-3), 1), "shot_strings_over_sample": round(ss_ms / dist["sample_ms"], 4),
            "shot_strings_mirror_ms": round(mirror_ms, 3), "shot_strings_mirror_states": int(min(8, npts)),
            "shot_strings_mirror_equal": bool(np.array_equal(mirror_rho, rho_hat[:8])), "median_offdiag_pqk_shot_window": float(np.median(KSS[off])),
        })
    if args.window > 0:
        W = args.window
        ctx.window_rdms(xs, W)  # warm-up
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            rho = ctx.window_rdms(xs, W)
            ts.append(1e3 * (time.perf_counter() - t0))
        win_ms = float(np.median(ts))
        KW, wgram_ms = timed(lambda: ctx.projected_window_gram(rho), args.reps)
        wflops = window_flops(info["dims"], W)
        dist.update({
            "window_width": W, "n_windows": int(rho.shape[1]), "window_reps": args.reps, "window_rdms_ms": round(win_ms, 3),
            "window_rdms_ms_min": round(min(ts), 3), "window_rdms_ms_max": round(max(ts), 3), "window_flops": wflops,
            "window_tflops": round(wflops / (win_ms * 1e-3) / 1e12, 3), "projected_window_gram_ms": round(wgram_ms, 3),
            "window_over_pair": round(win_ms / pair_ms, 4), "median_offdiag_pqk_window": float(np.median(KW[off])),
        })
    if args.amplitudes > 0:
        S_amp = args.amplitudes
        amp_bases = engine.random_bases(S_amp, n, 0)
        (amp_bits, lp_sample), amp_sample_ms = timed(lambda: ctx.sample(xs, S_amp, bases=amp_bases, seed=0, logp=True), args.reps)
        ctx.amplitudes(xs, amp_bits, bases=amp_bases, per_state=True, logp=True)  # warm-up
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            _, lp_amp = ctx.amplitudes(xs, amp_bits, bases=amp_bases, per_state=True, logp=True)
            ts.append(1e3 * (time.perf_counter() - t0))
        amp_ms = float(np.median(ts))
        aflops = amplitude_flops(info["dims"], S_amp)
        dist.update({
            "amp_strings": S_amp, "amp_reps": args.reps, "amplitudes_ms": round(amp_ms, 3), "amplitudes_ms_min": round(min(ts), 3),
            "amplitudes_ms_max": round(max(ts), 3), "amp_flops": aflops, "amp_tflops": round(aflops / (amp_ms * 1e-3) / 1e12, 3),
            "amp_sample_ms": round(amp_sample_ms, 3), "amp_over_sample": round(amp_ms / amp_sample_ms, 4),
            "max_abs_dlogp_amp_sample": float(np.abs(lp_amp - lp_sample).max()),
        })
    if args.mpo:
        def spread_ms(fn):
            fn()  # warm-up
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                out = fn()
                ts.append(1e3 * (time.perf_counter() - t0))
            return out, ts

        if args.mpo == "heisenberg":  # J_x XX + J_y YY + J_z ZZ on neighbours and a field h Z: 3 (n - 1) + n terms, bond 5
            terms = [(j, p + p, (k, k + 1)) for k in range(n - 1) for j, p in zip((1.0, 0.8, -0.6), "XYZ")] + [(0.5, "Z", (k,)) for k in range(n)]
            H = engine.mpo_from_terms(n, terms)
            n_terms, hulls = len(terms), sum(max(q) - min(q) + 1 for _, _, q in terms)
        else:  # sum_{i<j} 0.7^(j-i-1) Z_i Z_j: n (n - 1) / 2 terms, bond 3
            H = engine.mpo_exponential(n, "Z", "Z", 1.0, 0.7)
            terms, n_terms, hulls = None, n * (n - 1) // 2, sum((n - d) * (d + 1) for d in range(1, n))
        Vm, ts_h = spread_ms(lambda: ctx.mpo_expectations(xs, [H]))
        planes = int(H.bonds[:-1].sum())  # stacked planes of the first GEMM, summed over the sites
        dist.update({
            "mpo": args.mpo, "mpo_bond": H.max_bond(), "mpo_terms": n_terms, "mpo_reps": args.reps, "mpo_ms": round(float(np.median(ts_h)), 3),
            "mpo_ms_min": round(min(ts_h), 3), "mpo_ms_max": round(max(ts_h), 3), "mpo_plane_sites": planes, "mpo_terms_sum_hulls": int(hulls),
            "mpo_expected_work_ratio": round(planes / hulls, 4), "mpo_max_abs_value": float(np.abs(Vm).max()),
        })
        if terms is not None:
            coeff = np.array([c for c, _, _ in terms], dtype=np.complex128)
            specs = [(names, qubits) for _, names, qubits in terms]
            Vt, ts_t = spread_ms(lambda: ctx.operator_expectations(xs, specs) @ coeff)
            dist.update({
                "mpo_terms_ms": round(float(np.median(ts_t)), 3), "mpo_terms_ms_min": round(min(ts_t), 3), "mpo_terms_ms_max": round(max(ts_t), 3),
                "mpo_over_terms": round(float(np.median(ts_h)) / float(np.median(ts_t)), 4), "max_abs_d_mpo_terms": float(np.abs(Vm[:, 0] - Vt).max()),
            })
    if args.apply:
        def spread_apply(fn, keep=False):
            """ms of `reps` calls after one warm-up call; the sets the calls return are closed outside the timed window"""
            fn().close()
            ts, out = [], None
            for r in range(args.reps):
                t0 = time.perf_counter()
                out = fn()
                ts.append(1e3 * (time.perf_counter() - t0))
                if not (keep and r == args.reps - 1):
                    out.close()
            return out, ts

        if args.apply == "parity":
            O = engine.mpo_parity_projector(n, +1)
        elif args.apply == "heisenberg_step":  # 1 - i tau H, tau = 0.05, H the chain of --mpo heisenberg: bond 6
            terms = [(j, p + p, (k, k + 1)) for k in range(n - 1) for j, p in zip((1.0, 0.8, -0.6), "XYZ")] + [(0.5, "Z", (k,)) for k in range(n)]
            O = engine.Mpo([np.eye(2).reshape(1, 1, 2, 2)] * n) + engine.mpo_from_terms(n, terms).scale(-0.05j)
        else:
            g = np.random.default_rng(7)
            q, r = np.linalg.qr(g.standard_normal((4, 4)) + 1j * g.standard_normal((4, 4)))
            O = engine.mpo_two_qubit_gate(n, 0, n - 1, q * (np.diag(r) / np.abs(np.diag(r)))[None, :])
        # a product bond is at most 512 and the product is allocated whole: where the states are too wide for this MPO, or the
        # product image would pass --apply-max-gib, the states are capped first (reported as apply_source_cap), halving the cap
        def product_bytes(dims):
            pad = (O.bonds[None, :].astype(np.int64) * dims + 15) // 16 * 16
            return int(32 * (pad[:, :-1] * pad[:, 1:]).sum())

        src, cap, dims_src = xs, None, info["dims"].astype(np.int64)
        while int((O.bonds[None, :] * dims_src).max()) > 512 or product_bytes(dims_src) > args.apply_max_gib * 2**30:
            cap = 512 // O.max_bond() if cap is None else cap // 2
            if cap < 1:
                raise SystemExit("--apply: no bond cap brings the product under --apply-max-gib")
            dims_src = np.minimum(info["dims"].astype(np.int64), cap)
        if cap is not None:
            src = ctx.compress(xs, max_bond=cap)
        ps, ts_a = spread_apply(lambda: ctx.apply_mpo(src, O), keep=True)
        product_dims = ps.dims.copy()
        written = 8 * ps.image()[0]
        read = int(32 * (O.bonds[None, :-1].astype(np.int64) * src.dims[:, :-1].astype(np.int64) * src.dims[:, 1:]).sum())  # every true source element once per u
        cs, ts_c = spread_apply(lambda: ctx.compress(ps, max_discard=0.0), keep=True)
        apply_ms = float(np.median(ts_a))
        dist.update({
            "apply": args.apply, "apply_mpo_bond": O.max_bond(), "apply_source_cap": cap, "apply_source_max_bond": int(src.dims.max()), "apply_reps": args.reps,
            "apply_ms": round(apply_ms, 3), "apply_ms_min": round(min(ts_a), 3), "apply_ms_max": round(max(ts_a), 3),
            "apply_bytes_written": int(written), "apply_bytes_read": read, "apply_gbps": round(written / (apply_ms * 1e-3) / 1e9, 1),
            "apply_compress_ms": round(float(np.median(ts_c)), 3), "apply_compress_ms_min": round(min(ts_c), 3), "apply_compress_ms_max": round(max(ts_c), 3),
            "product_max_bond": int(product_dims.max()), "compressed_max_bond": int(cs.dims.max()),
        })
        cs.close(), ps.close()
        if src is not xs:
            src.close()
    print(json.dumps({
        "config": args.config, "n_qubits": n, "layers": reps, "gamma": gamma, "n_states": npts,
        "max_bond": int(info["dims"].max()), "build_s": round(build_s, 3),
        "gram_ms": round(gram_ms, 3), "local_paulis_ms": round(local_ms, 3), "projected_gram_ms": round(pgram_ms, 3),
        "local_pair_paulis_ms": round(pair_ms, 3), "projected_pair_gram_ms": round(pgram2_ms, 3),
        "local_over_gram": round(local_ms / gram_ms, 4), "pair_over_local": round(pair_ms / local_ms, 4),
        "local_flops": flops, "local_tflops": round(flops / (local_ms * 1e-3) / 1e12, 3),
        "pair_flops": flops2, "pair_tflops": round(flops2 / (pair_ms * 1e-3) / 1e12, 3),
        "median_offdiag_fidelity_K": float(np.median(K[off])), "median_offdiag_pqk": float(np.median(KP[off])),
        "median_offdiag_pqk2": float(np.median(KP2[off])), **dist,
    }), flush=True)
    xs.close()
    ctx.close()


if __name__ == "__main__":
    main()
