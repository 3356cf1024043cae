#!/usr/bin/env python3
"""Time ``Context.seed`` on one MI355X, in one process: the config's states built by the device builder (a set that records its
centre), then, each after a warm-up, ``ctx.seed(xs)`` (the verbatim path: one pass over the set's bytes), ``ctx.seed(xs,
sweep=True)`` (the sweep path: finite check, canonical sweep, gather) and, next to it, ``ctx.compress(xs)`` with no cap on the same
set (the sweep path should cost what that call costs, plus one copy).  Prints one JSON line: the median of each over the
repetitions with its minimum and maximum, the bytes of the set's image and of the seed's heap, and the largest bond.
usage: python tools/seed_time.py [--config cfg3|cfg4|cfg5] [--gamma G] [--reps N]"""
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


def timed(fn, reps):
    """(last result's summary, median ms, min ms, max ms) of ``fn``, whose result is closed, after one warm-up call."""
    fn()[0].close()
    ts, note = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out, note = fn()
        ts.append(time.perf_counter() - t0)
        out.close()
    return note, round(1e3 * float(np.median(ts)), 3), round(1e3 * min(ts), 3), round(1e3 * max(ts), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4", choices=("cfg3", "cfg4", "cfg5"))
    ap.add_argument("--gamma", type=float, default=None, help="default 1.0 (0.1 for cfg5)")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    gamma = args.gamma if args.gamma is not None else (0.1 if args.config == "cfg5" else 1.0)
    n, reps, d, npts = bench.CONFIGS[args.config]
    X = synthetic_features(npts, n, 5)
    ans = Q.KernelStateAnsatz(n, reps, gamma, Q.entanglement_graph(n, d))
    ctx = engine.Context(0)
    t0 = time.perf_counter()
    xs, _, info = ctx.build_share([ans.circuit_for_data(x) for x in X], 1.0 - 1e-16, max_bond=320)
    if xs is None:
        raise SystemExit(f"{len(info['dropped'])} states outgrew the device builder's bond cap")
    build_s = time.perf_counter() - t0
    ctx.trim()

    def seed(sweep):
        s = ctx.seed(xs, sweep=sweep)
        i = s.info(0)
        return s, (int(i["heap_bytes"]), float(i["fidelity"].min()), float(np.abs(i["norm"] - 1).max()), int(i["dims"].max()))

    def compress():
        c = ctx.compress(xs)
        return c, int(c.dims.max())

    verb, verb_ms, verb_lo, verb_hi = timed(lambda: seed(False), args.reps)
    swp, sweep_ms, sweep_lo, sweep_hi = timed(lambda: seed(True), args.reps)
    cbond, comp_ms, comp_lo, comp_hi = timed(compress, args.reps)
    image = int(xs.info()["device_bytes"])
    print(json.dumps({
        "config": args.config, "gamma": gamma, "n_states": npts, "n_qubits": n, "max_bond": int(info["dims"].max()), "build_s": round(build_s, 3), "centre": xs.centre,
        "set_image_bytes": image, "seed_heap_bytes": verb[0],
        "seed_verbatim_ms": verb_ms, "seed_verbatim_ms_min": verb_lo, "seed_verbatim_ms_max": verb_hi,
        "seed_verbatim_gb_per_s": round((image + verb[0]) / (verb_ms * 1e-3) / 1e9, 2),
        "seed_sweep_ms": sweep_ms, "seed_sweep_ms_min": sweep_lo, "seed_sweep_ms_max": sweep_hi, "seed_sweep_min_fidelity": swp[1], "seed_sweep_max_abs_norm_minus_1": swp[2],
        "seed_sweep_max_bond": swp[3],
        "compress_ms": comp_ms, "compress_ms_min": comp_lo, "compress_ms_max": comp_hi, "compress_max_bond": cbond,
        "sweep_over_compress": round(sweep_ms / comp_ms, 4), "reps": args.reps,
    }))
    xs.close()
    ctx.close()


if __name__ == "__main__":
    main()
