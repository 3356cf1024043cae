#!/usr/bin/env python3
"""What the segmentation of the site-fused sweep's chains executes, per launch of a bench config: steps and matrix instructions per
pair with no merged steps (QK_MERGE=0), with every admissible merge of the fixed pairs (k + 2 t, k + 2 t + 1) (QK_MERGE=1) and with
merges at either parity chosen per pair by dynamic programming (QK_MERGE=2, the default) -- and the device bytes of the merged images
the last two need.  The residency of X per kind of step (qk_resident: side by side, in place, partially resident, evicted whole, strips), what the
two parts of the rule move to the LDS form of phase 1 and what is still copied to the global buffer.  On top of QK_MERGE=2: the association of the steps (QK_ASSOC; tools/assoc_capi.cpp) -- matrix instructions, steps and
switches per pair with orientation 0 throughout (QK_ASSOC=0) and with the orientation chosen per step (the default), at the shipped
switch price and at 0 and 150.

The numbers come from the function the device runs (qk_segment_chain, csrc/qk_plan.h), compiled for the host from
tools/segment_capi.cpp and called through ctypes, over ALL pairs of the config's real plan (the host planner: class split, orientation
and edge_k as a Gram of the set gets them).  Matrix instructions as the kernels issue them: tiles of 16, K trimmed to the true bond in
steps of 4, three real products per complex one; the edge products (the same under every rule) are listed beside the steps.

    python tools/merge_potential.py [cfg4] [edge_k]     (CPU only; builds or loads the config's states like bench.py)
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {  # launch shape -> (elements of the LDS X buffer, units of one round, pairs of tiles per unit): csrc/qkgram.hip, seg_rule_of
    "12-wave dual (XCAP 8192)": (8192, 12, 1),
    "12-wave one-tile (XCAP 8192)": (8192, 24, 0),
    "8-wave one-tile (XCAP 4608)": (4608, 8, 0),
}
_lib = None


def segment_lib():
    """The host build of tools/segment_capi.cpp (made once per process in a temporary directory)."""
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="qk_segment_")
        so = os.path.join(tmp, "libqksegment.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "segment_capi.cpp")], check=True)
        _lib = C.CDLL(so)
        _lib.qk_segment_pairs.restype = None
        _lib.qk_segment_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64] + [C.c_int32] * 6 + [C.c_void_p] * 3
    return _lib


def segment_pairs(x_true, y_true, pairs, ek, shape, parities, greedy):
    """(masks [pairs][2] uint64, matrix instructions [pairs], steps [pairs]) of the pairs (x state, y state) under a launch shape."""
    x_true = np.ascontiguousarray(x_true, dtype=np.int32)
    y_true = np.ascontiguousarray(y_true, dtype=np.int32)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32)
    n = pairs.shape[0]
    masks, instr, steps = np.zeros((n, 2), dtype=np.uint64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
    xcap, cap, dual = SHAPES[shape]
    segment_lib().qk_segment_pairs(x_true.ctypes.data, y_true.ctypes.data, x_true.shape[1] - 1, pairs.ctypes.data, n, int(ek), xcap, cap, dual, int(parities), int(bool(greedy)),
                                   masks.ctypes.data, instr.ctypes.data, steps.ctypes.data)
    return masks, instr, steps


_assoc = None
ASSOC_FLAGS = {"starts_o1": 1, "ends_o1": 2, "first_step": 4, "last_step": 8, "merged_step": 16, "strip_between": 32, "one_round_step": 64, "pingpong_step": 128}  # tools/assoc_capi.cpp
SWITCH_PRICE = 40  # csrc/qk_plan.h: QK_SWITCH_PRICE


def assoc_lib():
    """The host build of tools/assoc_capi.cpp (made once per process in a temporary directory)."""
    global _assoc
    if _assoc is None:
        tmp = tempfile.mkdtemp(prefix="qk_assoc_")
        so = os.path.join(tmp, "libqkassoc.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "assoc_capi.cpp")], check=True)
        _assoc = C.CDLL(so)
        _assoc.qk_assoc_pairs.restype = None
        _assoc.qk_assoc_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64] + [C.c_int32] * 6 + [C.c_void_p] * 5
    return _assoc


def assoc_pairs(x_true, y_true, pairs, ek, shape, assoc, switch_price=SWITCH_PRICE):
    """The segmentation WITH the association of the steps (QK_MERGE=2; assoc as QK_ASSOC): (masks [pairs][4] uint64 -- merges, orientations --,
    matrix instructions [pairs], steps [pairs], switches [pairs], flags [pairs]: ASSOC_FLAGS) under a launch shape."""
    x_true = np.ascontiguousarray(x_true, dtype=np.int32)
    y_true = np.ascontiguousarray(y_true, dtype=np.int32)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32)
    n = pairs.shape[0]
    masks, instr = np.zeros((n, 4), dtype=np.uint64), np.zeros(n, dtype=np.int64)
    steps, switches, flags = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    xcap, cap, dual = SHAPES[shape]
    assoc_lib().qk_assoc_pairs(x_true.ctypes.data, y_true.ctypes.data, x_true.shape[1] - 1, pairs.ctypes.data, n, int(ek), xcap, cap, dual, int(assoc), int(switch_price),
                               masks.ctypes.data, instr.ctypes.data, steps.ctypes.data, switches.ctypes.data, flags.ctypes.data)
    return masks, instr, steps, switches, flags


ONESUM_CASES = {"nn_1": 1, "nn_2": 2, "nn_odd": 4, "nn_even": 8, "kmax_1": 16, "kmax_2": 32, "kmax_3": 64, "kmax_4": 128, "single_tile": 256, "tile_pair": 512,
                "plain_step": 1024, "merged_step": 2048, "strip_step": 4096}  # tools/assoc_capi.cpp: qk_onesum_pairs


def onesum_pairs(x_true, y_true, pairs, ek, shape, assoc, switch_price=SWITCH_PRICE):
    """What the column blocks of phase 2 meet on the chains of the pairs (segmentation and association as assoc_pairs makes them):
    (cases [pairs][2] -- ONESUM_CASES of the ordinary steps, of the switch steps --, blocks [pairs][2]: column blocks of the ordinary and of
    the switch steps, per unit of the shape) under a launch shape."""
    x_true = np.ascontiguousarray(x_true, dtype=np.int32)
    y_true = np.ascontiguousarray(y_true, dtype=np.int32)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32)
    n = pairs.shape[0]
    cases, blocks = np.zeros((n, 2), dtype=np.int32), np.zeros((n, 2), dtype=np.int64)
    xcap, cap, dual = SHAPES[shape]
    fn = assoc_lib().qk_onesum_pairs
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64] + [C.c_int32] * 6 + [C.c_void_p] * 2
    fn(x_true.ctypes.data, y_true.ctypes.data, x_true.shape[1] - 1, pairs.ctypes.data, n, int(ek), xcap, cap, dual, int(assoc), int(switch_price), cases.ctypes.data, blocks.ctypes.data)
    return cases, blocks


RESIDENT_CASES = {"part_x_low": 1, "part_x_top": 2, "part_low_top_in_a_row": 4, "keeps_one": 8, "keeps_all_but_one": 16, "keeps_none": 32, "merged_part": 64,
                  "part_then_not_resident": 128, "not_resident_then_part": 256, "ragged_part": 512, "ragged_panel_stays": 1024, "ragged_panel_evicted": 2048,
                  "side_by_side_in_large_only": 4096, "part_switches": 8192}  # tools/assoc_capi.cpp: qk_resident_pairs
RESIDENT_STATS = ("side", "in_place", "partial", "evicted_whole", "strips", "p1_lds_of_partial", "copied", "panels_of_partial", "panels_kept", "p1_of_partial")
RCAP = {"12-wave dual (XCAP 8192)": 9728, "12-wave one-tile (XCAP 8192)": 9728, "8-wave one-tile (XCAP 4608)": 4608}  # csrc/qk_plan.h: QKF_RCAP_ONE (checked in resident_pairs), QKF_XCAP_TWO


def resident_pairs(x_true, y_true, pairs, ek, shape, assoc, rcap=None, partial=True, merge=True, switch_price=SWITCH_PRICE):
    """The residency of X (csrc/qk_plan.h: qk_resident) along the chains of the pairs, walked as the kernels walk them: (cases [pairs] --
    RESIDENT_CASES --, stats [pairs][10] -- RESIDENT_STATS: matrix instructions per kind of step, the phase-1 matrix instructions of partially
    resident steps that run the LDS form, elements copied to the global buffer, panels of the partially resident steps and how many stay).
    rcap: elements the residency may use (None: the shape's shipped buffer; the shape's XCAP: the fallback instantiation); partial: QKF_RES_PARTIAL;
    merge False: QK_MERGE=0 (every site its own step, orientation 0)."""
    x_true = np.ascontiguousarray(x_true, dtype=np.int32)
    y_true = np.ascontiguousarray(y_true, dtype=np.int32)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32)
    n = pairs.shape[0]
    cases, stats = np.zeros(n, dtype=np.int32), np.zeros((n, len(RESIDENT_STATS)), dtype=np.int64)
    xcap, cap, dual = SHAPES[shape]
    lib = assoc_lib()
    fn = lib.qk_resident_pairs
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64] + [C.c_int32] * 9 + [C.c_void_p] * 2
    lib.qk_rcap_one.restype = C.c_int32
    assert lib.qk_rcap_one() == RCAP["12-wave dual (XCAP 8192)"], "RCAP is out of step with csrc/qk_plan.h"
    fn(x_true.ctypes.data, y_true.ctypes.data, x_true.shape[1] - 1, pairs.ctypes.data, n, int(ek), xcap, cap, dual, int(RCAP[shape] if rcap is None else rcap), int(bool(partial)),
       3 if merge else 0, int(assoc), int(switch_price), cases.ctypes.data, stats.ctypes.data)
    return cases, stats


def resident_table(dims, pairs, ek, shape, assoc=1):
    """The lines of the residency table of one launch: the parent's rule (the segmentation's buffer, no partial residency), each part alone, both."""
    xcap = SHAPES[shape][0]
    out = []
    for name, rcap, partial in (("parent", xcap, False), ("partial", xcap, True), ("large buffer", RCAP[shape], False), ("both (shipped)", RCAP[shape], True)):
        if rcap == xcap and name == "large buffer":
            continue  # (this shape has no larger buffer)
        _, st = resident_pairs(dims, dims, pairs, ek, shape, assoc, rcap, partial)
        t = st.sum(axis=0).astype(np.float64)
        total = t[:5].sum()
        out.append(f"  residency, {name:14s} (buffer {rcap}): matrix instr. side by side {t[0] / total * 100:5.1f} %, in place {t[1] / total * 100:6.3f} %, partially resident {t[2] / total * 100:5.1f} %, "
                   f"evicted whole {t[3] / total * 100:5.1f} %, strips {t[4] / total * 100:5.1f} %; panels that stay {t[8] / max(t[7], 1) * 100:5.1f} %; phase-1 instr. moved to the LDS form "
                   f"{t[5] / total * 100:5.2f} % of the launch ({t[5]:.3e}); elements copied per pair {t[6] / len(pairs):9.0f}")
    return out


def merged_steps(masks):
    """merged steps per pair: the bits of its mask (the first two words)"""
    return np.array([bin(int(r[0])).count("1") + bin(int(r[1])).count("1") for r in masks])


RULES = (("QK_MERGE=0", 0, True), ("QK_MERGE=1", 1, True), ("QK_MERGE=2", 3, False))  # name, allowed parities, every admissible merge / dynamic programme


def main():
    import bench
    from qml_cutensornet_amd import engine

    cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg4"
    n, reps, d, npts = bench.CONFIGS[cfg]
    gamma = 0.1 if cfg == "cfg5" else 1.0
    states, _ = bench.build_or_load_states(cfg, n, reps, d, gamma, npts, 5, 0, 1, os.cpu_count() or 1)
    dims = np.array([m.bond_dims() for m in states], dtype=np.int32)
    plan = engine.Plan(dims, None, 1, 0, 0, False)
    pairs, n_first = plan.pairs(), plan.first_run
    n_first = n_first() if callable(n_first) else n_first
    ek = int(sys.argv[2]) if len(sys.argv) > 2 else plan.edge_sites
    ek = ek() if callable(ek) else ek
    np_ = pairs.shape[0]
    print(f"{cfg}: {npts} states, {n} sites, max bond mean {dims.max(axis=1).mean():.1f} max {dims.max()}, {np_} pairs, first run {n_first}, edge_k {ek}")
    p16 = lambda v: (v.astype(np.int64) + 15) // 16 * 16  # noqa: E731
    pd = p16(dims)
    starts = n - 2 * ek - 1
    img = {1: sum(int((4 * pd[:, ek + s] * pd[:, ek + s + 2]).sum()) for s in range(starts)) * 16,
           2: sum(int((4 * pd[:, ek + s] * pd[:, ek + s + 2]).sum()) for s in range(0, starts, 2)) * 16}
    print(f"merged image of the set: even starts {img[2] / 2**30:.3f} GiB, every start {img[1] / 2**30:.3f} GiB (+{(img[1] - img[2]) / 2**30:.3f} GiB)")
    if ek > 0:  # the two edge products of a pair: tiles(a) tiles(b) 2^k / 4 k-steps x 3, at either end
        t = lambda v: (v.astype(np.int64) + 15) // 16  # noqa: E731
        edge = 3 * (2**ek // 4) * (t(dims[pairs[:, 0], ek]) * t(dims[pairs[:, 1], ek]) + t(dims[pairs[:, 0], n - ek]) * t(dims[pairs[:, 1], n - ek]))
    else:
        edge = np.zeros(np_, dtype=np.int64)
    split = 0 < n_first < np_
    runs = [("12-wave dual (XCAP 8192)", slice(0, n_first)), ("8-wave one-tile (XCAP 4608)", slice(n_first, np_))] if split else [(s, slice(0, np_)) for s in SHAPES]
    if not split:
        print("(one class of pairs: every shape is listed over all pairs; the launch takes one of them)")
    for shape, sl in runs:
        print(f"{shape}: {pairs[sl].shape[0]} pairs, edge products {edge[sl].mean():.0f} matrix instructions per pair")
        base = None
        for name, par, greedy in RULES:
            masks, instr, steps = segment_pairs(dims, dims, pairs[sl], ek, shape, par, greedy)
            cost = instr.mean() + 375.0 * steps.mean()
            if name == "QK_MERGE=1":
                base = (instr.mean(), cost, (instr + edge[sl]).mean())
            rel = "" if base is None or name == "QK_MERGE=1" else (f"  ({(instr.mean() / base[0] - 1) * 100:+.2f} % instr., {(cost / base[1] - 1) * 100:+.2f} % modelled cost, "
                                                                   f"{((instr + edge[sl]).mean() / base[2] - 1) * 100:+.2f} % instr. with the edges, against QK_MERGE=1)")
            odd = int(sum(bin(int(a) & 0xAAAAAAAAAAAAAAAA).count("1") + bin(int(b) & 0xAAAAAAAAAAAAAAAA).count("1") for a, b in masks))
            print(f"  {name}: steps/pair {steps.mean():6.2f}  merged {merged_steps(masks).mean():6.2f} (odd starts {odd / masks.shape[0]:5.2f})  matrix instr./pair {instr.mean():9.0f}"
                  f"  instr. + 375/step {cost:9.0f}{rel}")
        # the association of the steps (QK_ASSOC; on top of QK_MERGE=2): orientation 0 throughout against the choice per step
        base = None
        for name, assoc, price in (("QK_ASSOC=0", 0, SWITCH_PRICE), ("QK_ASSOC=1", 1, SWITCH_PRICE), ("QK_ASSOC=1 price 0", 1, 0), ("QK_ASSOC=1 price 150", 1, 150)):
            masks, instr, steps, switches, flags = assoc_pairs(dims, dims, pairs[sl], ek, shape, assoc, price)
            cost = instr.mean() + 375.0 * steps.mean() + price * switches.mean()
            if base is None:
                base = (instr.mean(), cost, (instr + edge[sl]).mean())
            rel = "" if assoc == 0 else (f"  ({(instr.mean() / base[0] - 1) * 100:+.2f} % instr., {(cost / base[1] - 1) * 100:+.2f} % modelled cost, "
                                         f"{((instr + edge[sl]).mean() / base[2] - 1) * 100:+.2f} % instr. with the edges, against QK_ASSOC=0)")
            print(f"  {name:20s}: steps/pair {steps.mean():6.2f}  merged {merged_steps(masks).mean():6.2f}  switches/pair {switches.mean():5.2f} (pairs that switch {(switches > 0).mean() * 100:5.1f} %, "
                  f"start in orientation 1 {((flags & 1) != 0).mean() * 100:5.1f} %, end in it {((flags & 2) != 0).mean() * 100:5.1f} %)  matrix instr./pair {instr.mean():9.0f}{rel}")
        # the residency of X (qk_resident; on top of QK_MERGE=2, QK_ASSOC=1): share of the matrix instructions per kind of step, under the parent's rule and the two parts
        for line in resident_table(dims, pairs[sl], ek, shape):
            print(line)
    plan.close()


if __name__ == "__main__":
    main()
