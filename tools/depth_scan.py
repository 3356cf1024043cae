#!/usr/bin/env python3
"""What a depth scan saves on one MI355X, in one process: the config's circuits are built ONCE to the deepest of the given depths with
a snapshot at the end of each depth's last layer (ctx.build_mps_scan), then once per depth the plain way (ctx.build_mps_set of the
depth-r circuits), and the Grams of the two are compared.  Prints one JSON line: scan_build_s, separate_build_s (a list) and its sum,
scan_over_separate, the largest bond and the heap bytes of every depth, and max |K_scan - K_separate| per depth.
usage: python tools/depth_scan.py cfg3|cfg4|cfg5 depth [depth ...] [--states N] [--gamma G]"""
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
from qml_cutensornet_amd.ansatz import check_depths  # noqa: E402
from qml_cutensornet_amd.data import synthetic_features  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", choices=("cfg3", "cfg4", "cfg5"))
    ap.add_argument("depths", type=int, nargs="+", help="layer counts, each at most the config's")
    ap.add_argument("--states", type=int, default=None, help="data points (default: the config's)")
    ap.add_argument("--gamma", type=float, default=None, help="default 1.0 (0.1 for cfg5)")
    ap.add_argument("--max-bond", type=int, default=320)
    args = ap.parse_args()
    gamma = args.gamma if args.gamma is not None else (0.1 if args.config == "cfg5" else 1.0)
    n, reps, d, npts = bench.CONFIGS[args.config]
    npts = args.states or npts
    depths = sorted(check_depths(args.depths, reps))
    X = synthetic_features(npts, n, 5)
    edges = Q.entanglement_graph(n, d)
    deep = Q.KernelStateAnsatz(n, depths[-1], gamma, edges)
    ends = deep.layer_ends()
    circuits = [deep.circuit_for_data(x) for x in X]
    ctx = engine.Context(0)
    # warm-up: the first launch of a process pays for loading the code object and for the context's arena
    ctx.build_mps_set(circuits[:1], max_bond=args.max_bond)[0].close()
    t0 = time.perf_counter()
    scan = ctx.build_mps_scan(circuits, [ends[r - 1] for r in depths], max_bond=args.max_bond)
    scan_s = time.perf_counter() - t0
    infos = [scan.info(j) for j in range(len(depths))]
    ctx.trim()
    K_scan = []
    for j in range(len(depths)):
        with scan.set(j) as xs:
            K_scan.append(ctx.gram(xs))
    scan.close()
    sep_s, dK = [], []
    for j, r in enumerate(depths):
        ans = Q.KernelStateAnsatz(n, r, gamma, edges)
        cs = [ans.circuit_for_data(x) for x in X]
        t0 = time.perf_counter()
        xs, _ = ctx.build_mps_set(cs, max_bond=args.max_bond)
        sep_s.append(time.perf_counter() - t0)
        ctx.trim()
        dK.append(float(np.abs(ctx.gram(xs) - K_scan[j]).max()))
        xs.close()
    print(json.dumps({
        "config": args.config, "n_qubits": n, "gamma": gamma, "n_states": npts, "depths": depths,
        "gates": [int(ends[r - 1]) for r in depths], "gate_count_ratio": round(sum(ends[r - 1] for r in depths) / ends[depths[-1] - 1], 3),
        "scan_build_s": round(scan_s, 3), "separate_build_s": [round(t, 3) for t in sep_s], "separate_build_sum_s": round(sum(sep_s), 3),
        "scan_over_separate": round(scan_s / sum(sep_s), 4),
        "max_bond": [int(i["dims"].max()) for i in infos], "heap_bytes": [int(i["heap_bytes"]) for i in infos],
        "max_abs_dK": dK,
    }), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
