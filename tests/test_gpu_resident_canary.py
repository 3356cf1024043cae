"""GPU tier: no stale value reaches a result through the residency of X (csrc/qk_plan.h: qk_resident) -- NaN canaries among the pairs of
a launch, the scheme of tests/test_gpu_canary.py on the rows of tests/test_gpu_resident.py.

A partially resident step leaves places that the next reader must not trust: the panels of X it sent to the global buffer (a
workgroup's slice of that buffer keeps them for its next pair) and the panels that stayed in LDS beside X' (the next step builds its X' over
them or beside them).  The probe is indirect, as in tests/test_gpu_canary.py: nothing is planted, a canary state (tests/helpers.py:
canary_copy -- the bond table of a clean state, nan + 1j nan in every element) makes every X, X' and evicted panel of ITS pairs NaN, in
LDS and in the workgroup's global buffers, wherever the rule puts them -- at either end of the buffer, so with the rows here both ends and
the evicted panels of every partially resident step are dirtied, while elements of the large buffer that no step of any pair writes are
dirtied by nobody and are not covered.  The sweep kernels are persistent, every workgroup here takes at least three pairs (asserted from
the stats), and canary pairs and clean pairs of the same bond rows follow each other on one workgroup.  Plans, segmentation and the
residency rule read bond tables alone, so the run with canaries walks the steps of the clean run: an entry without a canary must be the clean run's (the same bits for the DET forms,
1e-13 for the plain ones), an entry with one must be NaN, and the clean run after must be the clean run before (the same bits, 1e-14)."""
import numpy as np
import pytest

import helpers as H
import test_gpu_resident as R

pytestmark = pytest.mark.gpu

SWEEP_EPS = 1e-13   # between plain sweeps of different uploads
LAUNCH_EPS = 1e-14  # between two launches on the same buffers
SIZES = {"dual-large": 28, "dual-fallback": 28, "one-tile-large": 28, "one-tile-fallback": 28, "two-wg": 40}  # states per side: >= 3 pairs per workgroup on 256 CUs
X_CANARIES, Y_CANARIES = (2, 9, 17, 23), (4, 11, 20)  # rows 2, 3, 5, 5 of the x rows and 4, 5, 2 of the y rows
_cache = {}


def _lists(n):
    """(xs, ys) of n states each, cycling through the six rows (the same objects: an upload takes a state more than once), and the lists with canaries"""
    if n not in _cache:
        xs6, ys6, _ = R._sets()
        xs, ys = [xs6[i % len(xs6)] for i in range(n)], [ys6[(i + i // len(ys6)) % len(ys6)] for i in range(n)]
        _cache[n] = (xs, ys, H.with_canaries(xs, X_CANARIES), H.with_canaries(ys, Y_CANARIES))
    return _cache[n]


def _same(a, b, bits, eps):
    d = float(np.abs(a - b).max())
    return (np.array_equal(a, b) if bits else d < eps), d


@pytest.mark.parametrize("mode", ["merge0", "assoc1"])
@pytest.mark.parametrize("det", [False, True], ids=["plain", "det"])
@pytest.mark.parametrize("case", list(R.CASES))
def test_partial_residency_keeps_a_canary_to_its_pairs(built, monkeypatch, case, det, mode):
    from qml_cutensornet_amd import engine

    if det and mode == "assoc1":
        mode = "assoc0"  # (the ordered kernels run orientation 0 throughout)
    n = SIZES[case]
    xs, ys, xc, yc = _lists(n)
    kernel = R.set_env(monkeypatch, case, mode, det)
    runs = []
    with engine.context(0) as ctx:
        clean = (ctx.upload(xs), ctx.upload(ys))
        plan = engine.Plan(clean[0].dims, clean[1].dims)
        for rnd in range(3):  # clean, canaries (fresh uploads, the same plan object), clean again
            dx, dy = clean if rnd != 1 else (ctx.upload(xc), ctx.upload(yc))
            _, zz = ctx.gram_values_host(dx, dy, plan, want_z=True)
            st = ctx.stats()
            assert st["kernel_name"] == kernel and st["second_kernel"] == 0, (st["kernel_name"], st["second_kernel_name"])
            assert st["pairs"] == n * n and st["pairs"] >= 3 * st["grid"] > 0, st
            assert 16 * R.X_ELEMENTS[case] <= st["lds_bytes"] < 16 * R.X_ELEMENTS[case] + R.TABLE_ROOM, (case, st["lds_bytes"])
            pr = plan.pairs()
            z = np.full((n, n), np.nan + 0j)
            z[pr[:, 1], pr[:, 0]] = zz
            runs.append(z)
        pairs, ek = plan.pairs(), plan.edge_sites
        plan.close()
    # the chains of this launch meet the cases of the parity test (the same rows, every pair of them)
    rows = np.stack([pairs[:, 0] % len(R.X_ROWS), (pairs[:, 1] + pairs[:, 1] // len(R.Y_ROWS)) % len(R.Y_ROWS)], axis=1).astype(np.int32)
    got = R.visited(case, rows, ek)
    assert ek == R.EDGE and R.wanted(case) <= got, R.wanted(case) - got
    first, dirty, third = runs
    involved = H.canary_pair_mask(n, X_CANARIES, n, Y_CANARIES)
    assert np.isfinite(first).all() and np.isfinite(third).all()
    nan = np.isnan(dirty)
    assert np.array_equal(nan, involved), (f"{int((nan & ~involved).sum())} entries without a canary are NaN, {int((involved & ~nan).sum())} with one are not",
                                           np.argwhere(nan != involved)[:8].tolist())
    ok2, d2 = _same(dirty[~involved], first[~involved], det, SWEEP_EPS)
    ok3, d3 = _same(third, first, det, LAUNCH_EPS)
    print(f"canary {case}/{'det' if det else 'plain'}/{mode}: {st['kernel_name']}: grid {st['grid']}, pairs {st['pairs']}; canary pairs {int(involved.sum())}; worst clean-entry difference "
          f"{d2:.2e}, clean run after against before {d3:.2e}; {'bits asserted' if det else 'bounds 1e-13 / 1e-14'}")
    assert ok2, ("clean entries of the canary run against the clean run", d2)
    assert ok3, ("the clean run after the canary run against the one before", d3)
