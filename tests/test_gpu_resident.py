"""GPU tier: the residency of X in the site-fused sweep (csrc/qk_plan.h: qk_resident; csrc/qk_fused.h, the step loops) -- a step whose X
and X' each fit the LDS buffer but not together builds X' at the other end of the buffer, sends only the panels of X that X' overlaps to
the global buffer and lets the units of the panels that stay read X from LDS; the 12-wave shapes run with a larger buffer than the
segmentation counts on (QK_FUSED_BIG=0: the instantiation with the segmentation's buffer, which a launch with long tables falls back to);
which of the two ran is asserted from the launch's LDS bytes in the stats.

States: general-gauge twins (tests/helpers.py: scrambled) of random_mps on chains of 16 sites with QK_EDGE=4, so the sweep walks 8 sites;
six x rows and six y rows with true bonds of 20 .. 128 in the middle (most of them 64 .. 112: a b + a' b' passes the buffer while each
factor fits).  What the steps meet is ASSERTED from the function the device runs, compiled for the host (tools/merge_potential.py:
resident_pairs, which walks the chains as the kernels do), over the modes each case sweeps (QK_MERGE=0; QK_ASSOC=0 and 1 on the merges of
the dynamic programme):
  X at the low end and at the top in two partially resident steps in a row; a step that keeps exactly one panel, all but one, none; a
  merged step (pd = 4) with partial residency; a partially resident step directly followed by a step that is not LDS-resident (X evicted
  whole, X' in strips), and one directly preceded by a step that is not LDS-resident (its X came from the global buffer; its X' stayed whole
  in LDS -- behind a step whose X' leaves the LDS in several strips X is too large to be partially resident); a ragged true bond in a
  partially resident step (its last block of rows has fewer than 4 k-steps), with that block's panel staying and evicted; on the large
  buffer a step that is side by side only there, on the fallback none; and never a partially resident step that switches.
Cases: the 12-wave dual kernel, the 12-wave one-tile kernel (QK_FUSED_DUAL=0), each with the large buffer and with the fallback, and the
8-wave kernel.

z and |z|^2 of every mode against the oracle at 1e-11, and the plain forms against the DET forms of the same segmentation at 1e-13."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-11
SWEEP_EPS = 1e-13
N = 16
EDGE = 4
DUAL_NAME, ONE_NAME, TWO_NAME = "12-wave dual (XCAP 8192)", "12-wave one-tile (XCAP 8192)", "8-wave one-tile (XCAP 4608)"
CASES = {  # case: (switches, kernel, shape name of tools/merge_potential.py, elements the residency may use)
    "dual-large": ({"QK_FUSED_WGS": "1", "QK_FUSED_DUAL": "1", "QK_FUSED_BIG": "1"}, "qk_sweep_fused_dual_kernel<12, 8192, 3, {det}>", DUAL_NAME, None),
    "dual-fallback": ({"QK_FUSED_WGS": "1", "QK_FUSED_DUAL": "1", "QK_FUSED_BIG": "0"}, "qk_sweep_fused_dual_kernel<12, 8192, 3, {det}>", DUAL_NAME, 8192),
    "one-tile-large": ({"QK_FUSED_WGS": "1", "QK_FUSED_DUAL": "0", "QK_FUSED_BIG": "1"}, "qk_sweep_fused_kernel<12, 2, 8192, 3, {det}>", ONE_NAME, None),
    "one-tile-fallback": ({"QK_FUSED_WGS": "1", "QK_FUSED_DUAL": "0", "QK_FUSED_BIG": "0"}, "qk_sweep_fused_kernel<12, 2, 8192, 3, {det}>", ONE_NAME, 8192),
    "two-wg": ({"QK_FUSED_WGS": "2"}, "qk_sweep_fused_kernel<8, 1, 4608, 4, {det}>", TWO_NAME, None),
}
X_ELEMENTS = {"dual-large": 9728, "dual-fallback": 8192, "one-tile-large": 9728, "one-tile-fallback": 8192, "two-wg": 4608}  # of the X buffer of the instantiation that must run
TABLE_ROOM = 8192  # bytes behind the X buffer that hold the launch's tables at the most (csrc/qk_plan.h: QKF_META_ROOM)
MODES = {"merge0": {"QK_MERGE": "0"}, "assoc0": {"QK_ASSOC": "0"}, "assoc1": {"QK_ASSOC": "1"}}  # (QK_MERGE=0: every site a step of its own, orientation 0)
X_ROWS = [  # true bonds at the cuts 0 .. 16 (a bond is at most twice its neighbours)
    [1, 2, 4, 8, 16, 32, 64, 108, 80, 48, 64, 32, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 16, 32, 40, 76, 64, 56, 64, 32, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 16, 20, 32, 64, 108, 112, 64, 32, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 16, 32, 64, 96, 108, 112, 64, 32, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 16, 32, 64, 112, 80, 64, 40, 32, 16, 8, 4, 2, 1],  # with its y row: X of 112 x 96 from the global buffer, then 80 x 96 -> 64 x 64 partially resident
    [1, 2, 4, 8, 16, 32, 64, 64, 128, 64, 64, 32, 16, 8, 4, 2, 1],  # with its y row: 64 x 112 -> 128 x 64, an X' that leaves no panel of X room
]
Y_ROWS = [
    [1, 2, 4, 8, 16, 32, 64, 72, 100, 76, 64, 32, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 16, 32, 28, 48, 48, 32, 28, 32, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 16, 32, 60, 76, 96, 60, 60, 32, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 16, 32, 64, 60, 64, 56, 64, 32, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 16, 32, 64, 96, 96, 64, 40, 32, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 16, 32, 64, 112, 64, 64, 64, 32, 16, 8, 4, 2, 1],
]
_cache = {}


def potential():
    if "tool" not in _cache:
        spec = importlib.util.spec_from_file_location("merge_potential", os.path.join(ROOT, "tools", "merge_potential.py"))
        _cache["tool"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_cache["tool"])
    return _cache["tool"]


def all_pairs():
    return np.array([(i, j) for j in range(len(Y_ROWS)) for i in range(len(X_ROWS))], dtype=np.int32)


def visited(case, pairs=None, ek=EDGE):
    """the names of tool.RESIDENT_CASES the chains of the rows meet in the modes the case sweeps, from the host function"""
    tool = potential()
    _, _, shape, rcap = CASES[case]
    xd, yd = np.array(X_ROWS, dtype=np.int32), np.array(Y_ROWS, dtype=np.int32)
    pairs = all_pairs() if pairs is None else pairs
    seen = 0
    for merge, assoc in ((False, 0), (True, 0), (True, 1)):
        cases, _ = tool.resident_pairs(xd, yd, pairs, ek, shape, assoc, rcap=rcap, merge=merge)
        seen |= int(np.bitwise_or.reduce(cases))
    return {name for name, bit in tool.RESIDENT_CASES.items() if seen & bit}


def wanted(case):
    every = {"part_x_low", "part_x_top", "part_low_top_in_a_row", "keeps_one", "keeps_all_but_one", "keeps_none", "merged_part", "part_then_not_resident", "not_resident_then_part",
             "ragged_part", "ragged_panel_stays", "ragged_panel_evicted"}
    return every | ({"side_by_side_in_large_only"} if case.endswith("large") else set())


def never(case):
    return {"part_switches"} | (set() if case.endswith("large") else {"side_by_side_in_large_only"})


def _sets():
    """(xs, ys, z of the oracle [y][x]) -- made once for the module; read-only."""
    import qml_cutensornet_amd as Q
    from helpers import scrambled
    from oracle import c_oracle

    if "sets" not in _cache:
        rng = np.random.default_rng(1121)
        xs = [scrambled(Q.random_mps(N, row, rng), rng) for row in X_ROWS]
        ys = [scrambled(Q.random_mps(N, row, rng), rng) for row in Y_ROWS]
        assert [[int(b) for b in m.bond_dims()] for m in xs] == X_ROWS and [[int(b) for b in m.bond_dims()] for m in ys] == Y_ROWS
        _, z, _ = c_oracle.gram_pairs([m.tensors for m in xs], [m.tensors for m in ys], all_pairs(), 8)
        z = z.reshape(len(ys), len(xs))
        z.setflags(write=False)
        _cache["sets"] = (xs, ys, z)
    return _cache["sets"]


def set_env(monkeypatch, case, mode, det):
    for k in ("QK_FUSED_WGS", "QK_FUSED_DUAL", "QK_FUSED_BIG", "QK_MERGE", "QK_ASSOC", "QK_SWITCH_PRICE", "QK_FUSED_SPLIT", "QK_PLAN_ORIENT", "QK_GANG"):
        monkeypatch.delenv(k, raising=False)
    for k, v in list(CASES[case][0].items()) + list(MODES[mode].items()):
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("QK_FUSED", "2")
    monkeypatch.setenv("QK_PLAN_NO_MIXED", "1")
    monkeypatch.setenv("QK_EDGE", str(EDGE))
    monkeypatch.setenv("QK_DETERMINISTIC", "1" if det else "0")
    return CASES[case][1].format(det="true" if det else "false")


def _sweep(monkeypatch, case, mode, xs, ys, det=False):
    """(z [y][x], values [y][x], pairs, edge_k) of the rectangular Gram of xs and ys."""
    from qml_cutensornet_amd import engine

    kernel = set_env(monkeypatch, case, mode, det)
    with engine.context(0) as ctx, ctx.upload(xs) as dx, ctx.upload(ys) as dy:
        plan = engine.Plan(dx.dims, dy.dims, orient=False)
        vals, zz = ctx.gram_values_host(dx, dy, plan, want_z=True)
        st = ctx.stats()
        assert st["kernel_name"] == kernel, st["kernel_name"]
        # which instantiation ran: the launch's dynamic LDS is its X buffer and the chain's tables behind it (the name is the shape's for both)
        assert 16 * X_ELEMENTS[case] <= st["lds_bytes"] < 16 * X_ELEMENTS[case] + TABLE_ROOM and st["second_lds_bytes"] == 0, (case, st["lds_bytes"])
        pairs, ek = plan.pairs(), plan.edge_sites
        plan.close()
    z, v = np.full((len(ys), len(xs)), np.nan + 0j), np.full((len(ys), len(xs)), np.nan)
    z[pairs[:, 1], pairs[:, 0]], v[pairs[:, 1], pairs[:, 0]] = zz, vals
    return z, v, pairs, ek


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_partially_resident_steps_agree_with_the_oracle_and_the_ordered_kernels(built, monkeypatch, case):
    xs, ys, z_ref = _sets()
    out = {m: _sweep(monkeypatch, case, m, xs, ys) for m in MODES}
    det = {m: _sweep(monkeypatch, case, m, xs, ys, det=True) for m in ("merge0", "assoc0")}  # (the ordered kernels run orientation 0 throughout)
    pairs, ek = out["assoc1"][2], out["assoc1"][3]
    assert ek == EDGE and len(pairs) == len(xs) * len(ys)
    for m, (z, v, _, _) in list(out.items()) + [("det " + m, r) for m, r in det.items()]:
        zd, vd = det["merge0" if m.endswith("merge0") else "assoc0"][:2]
        print(f"{case} {m}: max |z - oracle| {np.abs(z - z_ref).max():.2e}, |values - oracle| {np.abs(v - np.abs(z_ref) ** 2).max():.2e}, |z - ordered| {np.abs(z - zd).max():.2e}")
        assert np.abs(z - z_ref).max() < TOL and np.abs(v - np.abs(z_ref) ** 2).max() < TOL, m
        assert np.abs(z - zd).max() < SWEEP_EPS and np.abs(v - vd).max() < SWEEP_EPS, m
    got = visited(case, pairs, ek)
    print(f"{case}: the steps meet {sorted(got)}")
    assert wanted(case) <= got, wanted(case) - got
    assert not (never(case) & got), never(case) & got
