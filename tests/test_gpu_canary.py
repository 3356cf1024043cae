"""GPU tier: no stale or foreign value reaches a result -- NaN canaries among the pairs of a launch, in the batch of a local sweep
and in the history of a context.

Every sweep kernel is persistent (a workgroup reuses its LDS, its registers and its slice of the X / T buffer for hundreds of pairs)
and a context keeps five device buffers between calls (qk_host.h: scratch, build_arena, build_work, derive_tmp, local_scratch --
the last one laid out differently by every local sweep).  The design leans on "the other operand's padding is zero" (K walked to the
true bond, M and N to the padded one), which holds only while whatever lies in a pad row, a K-tail or a slot gap is FINITE; the
rest of the suite hands on finite values of order 1, and a stale value times a zero pad is 0.  Here the probe is a canary state
(tests/helpers.py: canary_copy): the bond table of a clean state, nan + 1j nan in every element.  Plans, kernel choice, tiling,
segmentation, queues and batch cuts read bond tables alone (tests/test_canary_host.py), so a run with canaries walks the steps of
the clean run: a result that involves no canary must be the clean run's, a result that involves one must be NaN (the canary really
went through the kernel), and a clean call after a poisoned one must be the clean call before it.

  (a) a canary among the pairs of ONE launch: the cases and switches of tests/test_gpu_many_pairs.py (>= 3 pairs per workgroup,
      asserted from the stats), swept clean / with canaries (fresh uploads, the same plan object) / clean again on one context, with
      the tiled plan, with Context.overlaps (one queue) and with gram of the symmetric set;
  (b) a canary in the batch of a local sweep: the six gauge-scrambled twins with states 1 and 4 (and, as a placement of its own,
      state 3: the profile that reaches 128) replaced, and the two twins of bond 300 with one replaced;
  (c) a poisoned history: every entry point clean / a NaN-tolerant entry point on the ALL-canary copy of the set / clean again on
      one shared context, against the same call on a fresh context, and once more after Context.trim().

Bounds, all the project's own: the same bits for the DET sweeps and for every local entry point (documented bit-reproducible);
SWEEP_EPS = 1e-13 between plain sweeps of different uploads; LAUNCH_EPS = 1e-14 between two launches on the same buffers.  Every case
prints its worst difference; no bound was set by what was observed.

Measured on the MI355X: every case passes as the kernels stand.  The NaN entries are exactly the canary entries (400 of 864 pairs
on "fused12", 736 of 1600 on "fused8", 2944 of 6400 on "wave2", 5794 of 12544 on "wave", 990 of 2701 on "split"); clean entries of
the canary run against the clean run: 0 for the DET forms, the one-wave, small-bond and ring sweeps (double and float), at most
1.3e-15 for the plain fused forms (the Gram's |z|^2; 4e-17 on z); the clean run after against the one before: 0 and at most
1.3e-15.  Every local entry point: the same bits, in (b) and in (c), before and after trim().  The two-launch "mixed" set is the
one case whose first launch holds no clean pair (its pairs are those with state 112 or 113, and the placement makes both
canaries): it checks that launch's NaNs and what it leaves for the second launch.  tests/test_canary_host.py shows on a numpy
model of a persistent workgroup which defect the probe is for: a stale read that finite leftovers hide.

What is never done: no canary is an input of anything built on the Jacobi factorisations (the device builder, bond_spectra,
compress) -- as victims of (c) they run on finite data only.  What was read before the first run, for loops whose trip count could
depend on a tensor VALUE (a NaN never compares true, so such a loop could spin):
  * qk_fused.h: the pair loops end on qk_pull's queue index; site, strip, round and item loops run over the step table, which
    qkf_step_table makes from the bond tables; qkf_turn_add's wait reads an integer turn counter and gives up after 2^20 spins;
  * qk_ring.h: qk_sweep_ring_kernel / qk_sweep_small_kernel / the tile streams end on the pair counter and walk n_sites and the
    padded / true bonds staged per pair; zgemm_ring3's trip counts are M, N, K;
  * qk_local.hip: every launch is a list of (chain, block) tasks made on the host from the bond tables (qk_local_plan.h); the
    reductions run over chunk counts; qk_smp_draw_kernel and qk_amp_pick_kernel loop over lanes and the true bond -- a NaN total
    makes `ok` false (bit 0, v = 0, the chain's `bad` flag) and fmax drops a NaN, neither repeats anything.  sample meets a
    canary in one place only, the refusal test of (b), whose call fails as documented (QK_EDEVICE); it is no poisoner of (c);
  * qk_build_kernels.h: both Jacobi loops are `for (; sweep < MAX_SWEEPS; ++sweep)` (lines 71 and 562, MAX_SWEEPS = 40 in
    qk_build.hip) -- capped, and still never given a canary."""
import numpy as np
import pytest

import helpers as H
from test_gpu_many_pairs import CHAINS, DUAL, FUSED, LAUNCH_EPS, NOT_WAVE, OTHER, SWEEP_EPS, TWO, _set_env, _sweep_plan, _upload

pytestmark = pytest.mark.gpu

LOCAL_VARS = ("QK_STRINGS_BATCH", "QK_BLOCK_BATCH", "QK_SAMPLE_BATCH", "QK_AMP_BATCH", "QK_WINDOW_BATCH")


# ------------------------------------------------------------------------------------------------------------ shared checks
def _same(a, b, bits, eps):
    """(ok, worst difference) of two arrays of finite values: the same bits, or within eps."""
    a, b = np.asarray(a), np.asarray(b)
    if a.size == 0:
        return True, 0.0
    d = float(np.abs(a - b).max())
    return (np.array_equal(a, b) if bits else d < eps), d


def _three_runs(what, first, dirty, third, involved, have, bits):
    """One form of a case: ``first`` and ``third`` the clean sweeps, ``dirty`` the sweep with canaries, ``involved`` the entries
    that involve a canary, ``have`` the entries the plan lists.  Returns (canary entries, worst clean-entry difference of the
    canary run, worst difference of the third run)."""
    assert first.shape == dirty.shape == third.shape == involved.shape == have.shape, what
    assert not np.isnan(first[have]).any() and np.isfinite(first[have]).all(), (what, "the clean run is not finite")
    want, got = involved & have, np.isnan(dirty) & have
    n_want, n_got = int(want.sum()), int(got.sum())
    spoiled, missed = np.argwhere(got & ~want), np.argwhere(want & ~got)
    assert n_want > 0, what
    assert len(spoiled) == 0, (what, f"{len(spoiled)} entries without a canary are NaN", spoiled[:8].tolist())
    assert len(missed) == 0, (what, f"{len(missed)} entries with a canary are not NaN", missed[:8].tolist())
    assert n_got == n_want
    free = have & ~involved
    ok2, d2 = _same(dirty[free], first[free], bits, SWEEP_EPS)
    assert ok2, (what, "clean entries of the canary run against the clean run", d2, np.argwhere(free & (dirty != first))[:8].tolist())
    ok3, d3 = _same(third[have], first[have], bits, LAUNCH_EPS)
    assert ok3, (what, "the clean run after the canary run against the one before", d3)
    return n_want, d2, d3


def _line(tag, st, n_canary, worst, bits):
    second = f" + {st['second_kernel_name']}" if st.get("second_kernel") else ""
    print(f"canary {tag}: {st['kernel_name']}{second}: grid {st['grid']}, pairs {st['pairs']}, queues {st['queues']}; canary pairs {n_canary}; "
          f"worst clean-entry difference {worst[0]:.2e} (tiled plan / flat list / Gram: {', '.join(f'{d:.2e}' for d in worst[1])}), clean run after against before "
          f"{worst[2]:.2e}; {'bits asserted' if bits else 'bounds 1e-13 / 1e-14'}")


# ------------------------------------------------------------------------------------------------------------ (a) one launch
_sets = {}


def _rect_sets(name):
    """(xs, ys, sym, canary indices of the three) of a rectangular case and the same lists with canaries; made once."""
    if name not in _sets:
        xs, ys = H.many_pair_sets(name)
        sym = H.many_pair_symmetric(name, xs, ys)
        ix, iy = H.many_pair_canaries(name)
        isym = H.many_pair_symmetric_canaries(name)
        _sets[name] = (xs, ys, sym, ix, iy, isym, H.with_canaries(xs, ix), H.with_canaries(ys, iy), H.with_canaries(sym, isym))
    return _sets[name]


def _canary_case(monkeypatch, tag, name, env, kernel, queues, bits, f32=False):
    from qml_cutensornet_amd import engine

    xs, ys, sym, ix, iy, isym, xc, yc, sc = _rect_sets(name)
    nx, ny, ns = len(xs), len(ys), len(sym)
    _set_env(monkeypatch, env)
    runs = []
    with engine.context(0) as ctx:
        clean = [_upload(ctx, s, f32) for s in (xs, ys, sym)]
        plan = engine.Plan(clean[0].dims, clean[1].dims)
        assert plan.num_pairs == nx * ny
        for rnd in range(3):  # clean, canaries (fresh uploads, the same plan object), clean again
            dx, dy, ds = clean if rnd != 1 else [_upload(ctx, s, f32) for s in (xc, yc, sc)]
            z, st = _sweep_plan(ctx, dx, dy, plan)
            assert st["kernel_name"] == kernel and st["second_kernel"] == 0, (st["kernel_name"], st["second_kernel_name"])
            assert st["pairs"] == nx * ny and st["pairs"] >= 3 * st["grid"] > 0 and st["queues"] == queues, st
            z_flat = ctx.overlaps(dx, dy)  # the flat list: one queue
            st_flat = ctx.stats()
            assert st_flat["kernel_name"] == kernel and st_flat["pairs"] >= 3 * st_flat["grid"] > 0 and st_flat["queues"] == 1, st_flat
            K = ctx.gram(ds)
            st_sym = ctx.stats()
            assert st_sym["kernel_name"] == kernel and st_sym["second_kernel"] == 0 and st_sym["pairs"] >= 3 * st_sym["grid"] > 0, st_sym
            runs.append((z, z_flat, K))
        plan.close()
    rect, symm = H.canary_pair_mask(nx, ix, ny, iy), H.canary_pair_mask(ns, isym)
    all_r, all_s = np.ones((ny, nx), dtype=bool), np.ones((ns, ns), dtype=bool)
    n_z, d2_z, d3_z = _three_runs(f"{tag}: tiled plan", runs[0][0], runs[1][0], runs[2][0], rect, all_r, bits)
    n_f, d2_f, d3_f = _three_runs(f"{tag}: flat list", runs[0][1], runs[1][1], runs[2][1], rect, all_r, bits)
    n_K, d2_K, d3_K = _three_runs(f"{tag}: Gram", runs[0][2], runs[1][2], runs[2][2], symm, all_s, bits)
    _line(tag, st, n_z, (max(d2_z, d2_f, d2_K), (d2_z, d2_f, d2_K), max(d3_z, d3_f, d3_K)), bits)
    assert n_z == n_f == int(rect.sum()) and n_K == int(symm.sum())
    K2 = runs[1][2]  # K == K.T: the NaN rows AND the NaN columns
    assert np.array_equal(K2, K2.T, equal_nan=True) and np.isnan(K2[isym]).all() and np.isnan(K2[:, isym]).all()
    for K in (runs[0][2], runs[2][2]):
        assert np.array_equal(K, K.T)


@pytest.mark.parametrize("chain", list(CHAINS))
@pytest.mark.parametrize("det", [False, True], ids=["plain", "det"])
@pytest.mark.parametrize("shape", list(FUSED))
def test_fused_sweeps_keep_a_canary_to_its_pairs(built, monkeypatch, shape, det, chain):
    name, env, kernel = FUSED[shape]
    env = dict(env, QK_DETERMINISTIC="1" if det else "0", **CHAINS[chain])
    _canary_case(monkeypatch, f"{shape}/{'det' if det else 'plain'}/{chain}", name, env, kernel.format(det="true" if det else "false"), 8, bits=det)


@pytest.mark.parametrize("det", [False, True], ids=["plain", "det"])
def test_default_segmentation_keeps_a_canary_to_its_pairs(built, monkeypatch, det):
    """QK_MERGE unset: the segmentation chosen per pair by dynamic programming, on the edge blocks of QK_EDGE=4."""
    name, env, kernel = FUSED["dual"]
    env = dict(env, QK_DETERMINISTIC="1" if det else "0", QK_EDGE="4")
    assert "QK_MERGE" not in env
    _canary_case(monkeypatch, f"dual/{'det' if det else 'plain'}/merge-default", name, env, kernel.format(det="true" if det else "false"), 8, bits=det)


@pytest.mark.parametrize("case", list(OTHER))
def test_one_wave_small_and_ring_sweeps_keep_a_canary_to_its_pairs(built, monkeypatch, case):
    name, env, kernel, queues, f32 = OTHER[case]
    _canary_case(monkeypatch, case, name, env, kernel, queues, bits=False, f32=f32)


FLOAT = {  # complex64 ARITHMETIC (a complex64 set above the one-wave sweep's bonds, or with that sweep switched off): to_f32() of the upload
    "ring-float": ("fused8", dict(NOT_WAVE), "qk_sweep_ring_kernel<float>"),
    "small-float": ("wave2", dict(NOT_WAVE), "qk_sweep_small_kernel<float>"),
}


@pytest.mark.parametrize("case", list(FLOAT))
def test_complex64_sweeps_keep_a_canary_to_its_pairs(built, monkeypatch, case):
    name, env, kernel = FLOAT[case]
    _canary_case(monkeypatch, case, name, env, kernel, 1, bits=False, f32=True)


def _two_launch_canary_case(monkeypatch, tag, name, env, kernels, bits):
    """A symmetric Gram whose plan has two runs, each a launch of its own."""
    from qml_cutensornet_amd import engine

    xs = H.many_pair_gram_set(name)
    idx = H.many_pair_gram_canaries(name)
    xc = H.with_canaries(xs, idx)
    ns = len(xs)
    _set_env(monkeypatch, env)
    runs = []
    with engine.context(0) as ctx, ctx.upload(xs) as dx:
        plan = engine.Plan(dx.dims)
        second = plan.num_pairs - plan.first_run
        for rnd in range(3):
            d = dx if rnd != 1 else ctx.upload(xc)
            z, st = _sweep_plan(ctx, d, None, plan)
            firsts = kernels[0] if isinstance(kernels[0], tuple) else (kernels[0],)
            assert st["kernel_name"] in firsts and st["second_kernel_name"] == kernels[1], (st["kernel_name"], st["second_kernel_name"])
            kernels = (st["kernel_name"], kernels[1])  # every further launch: the same two
            assert st["queues"] == 8 and st["second_pairs"] == second > 0 and st["pairs"] == plan.num_pairs and st["pairs"] >= 3 * st["grid"] > 0, st
            K = ctx.gram(d)
            st_K = ctx.stats()
            assert (st_K["kernel_name"], st_K["second_kernel_name"]) == kernels and st_K["second_pairs"] == second
            runs.append((z, K))
        pr = plan.pairs()
        plan.close()
    have = np.zeros((ns, ns), dtype=bool)  # an oriented plan lists (i, j) or (j, i)
    have[pr[:, 1], pr[:, 0]] = True
    assert np.all(have | have.T) and have.sum() == len(pr)
    mask = H.canary_pair_mask(ns, idx)
    n_z, d2_z, d3_z = _three_runs(f"{tag}: plan", runs[0][0], runs[1][0], runs[2][0], mask, have, bits)
    n_K, d2_K, d3_K = _three_runs(f"{tag}: Gram", runs[0][1], runs[1][1], runs[2][1], mask, np.ones((ns, ns), dtype=bool), bits)
    in_second = np.zeros((ns, ns), dtype=bool)
    in_second[pr[len(pr) - second:, 1], pr[len(pr) - second:, 0]] = True
    parts = [(int((part & mask).sum()), int((part & ~mask).sum())) for part in (have & ~in_second, have & in_second)]  # (canary, clean) pairs of each launch
    # Both launches hold canary pairs, and the second one clean pairs.  The first launch of "split" holds clean pairs too; that of "mixed" cannot: its pairs
    # are those with state 112 or 113 (caps 90 and 140), and both are canaries -- 112 by the period, 113 as the largest cap -- so "mixed" checks the
    # NaNs of its first launch, what that launch leaves behind for the second one, and the clean pairs of the second.
    assert parts[0][0] > 0 and parts[1][0] > 0 and parts[1][1] > 0 and (parts[0][1] > 0 or name == "mixed"), parts
    print(f"canary {tag}: {kernels[0]} + {kernels[1]}: grid {st['grid']}, pairs {st['pairs'] - second} + {second}, queues {st['queues']}; canary pairs {n_z} of the plan "
          f"((canary, clean) of the two launches: {parts}), {n_K} of the Gram; worst clean-entry difference {max(d2_z, d2_K):.2e}, clean run after against before "
          f"{max(d3_z, d3_K):.2e}; {'bits asserted' if bits else 'bounds 1e-13 / 1e-14'}")
    K2 = runs[1][1]
    assert np.array_equal(K2, K2.T, equal_nan=True) and np.isnan(K2[idx]).all() and np.isnan(K2[:, idx]).all()


@pytest.mark.parametrize("det", [False, True], ids=["plain", "det"])
def test_split_sweep_keeps_a_canary_to_its_pairs(built, monkeypatch, det):
    d = "true" if det else "false"
    _two_launch_canary_case(monkeypatch, f"split/{'det' if det else 'plain'}", "split", {"QK_FUSED_SPLIT": "2", "QK_DETERMINISTIC": "1" if det else "0"},
                            (DUAL.format(det=d), TWO.format(det=d)), bits=det)


@pytest.mark.parametrize("det", [False, True], ids=["plain", "det"])
def test_mixed_set_keeps_a_canary_to_its_pairs(built, monkeypatch, det):
    d = "true" if det else "false"
    _two_launch_canary_case(monkeypatch, f"mixed/{'det' if det else 'plain'}", "mixed", {"QK_DETERMINISTIC": "1" if det else "0"},
                            ((DUAL.format(det=d), TWO.format(det=d)), "qk_sweep_wave2_kernel<3, double>"), bits=det)


@pytest.mark.parametrize("det", [False, True], ids=["plain", "det"])
def test_rank_shares_keep_a_canary_to_its_pairs(built, monkeypatch, det):
    from qml_cutensornet_amd import engine

    xs, ys, _, ix, iy, _, xc, yc, _ = _rect_sets("fused12-ranks")
    nx, ny, world = len(xs), len(ys), 3
    kernel = DUAL.format(det="true" if det else "false")
    _set_env(monkeypatch, dict(FUSED["dual"][1], QK_DETERMINISTIC="1" if det else "0", **CHAINS["edge4-merged"]))
    mask = H.canary_pair_mask(nx, ix, ny, iy)
    seen = np.zeros((ny, nx), dtype=bool)
    with engine.context(0) as ctx, ctx.upload(xs) as dx, ctx.upload(ys) as dy:
        for r in range(world):
            share = engine.Plan(dx.dims, dy.dims, world, r)
            runs = []
            for rnd in range(3):
                ex, ey = (dx, dy) if rnd != 1 else (ctx.upload(xc), ctx.upload(yc))
                z, st = _sweep_plan(ctx, ex, ey, share)
                assert st["kernel_name"] == kernel and st["pairs"] == share.num_pairs and st["pairs"] >= 3 * st["grid"] > 0, st
                runs.append(z)
                if rnd == 1:
                    ex.close(), ey.close()
            pr = share.pairs()
            share.close()
            have = np.zeros((ny, nx), dtype=bool)
            have[pr[:, 1], pr[:, 0]] = True
            assert not (have & seen).any()
            seen |= have
            n_c, d2, d3 = _three_runs(f"rank {r} of {world}", runs[0], runs[1], runs[2], mask, have, det)
            print(f"canary ranks/{'det' if det else 'plain'}: share {r}: {kernel}: grid {st['grid']}, pairs {st['pairs']}; canary pairs {n_c}; worst clean-entry difference "
                  f"{d2:.2e}, clean run after against before {d3:.2e}; {'bits asserted' if det else 'bounds 1e-13 / 1e-14'}")
    assert seen.all()


# ------------------------------------------------------------------------------------------------------------ (b) a local batch
def _strings(n):
    """A dozen strings: one of full support, the all-identity one, single sites at both ends, neighbours, far pairs, runs."""
    assert n >= 12
    return ["Z" * n, "I" * n, ("X", (0,)), ("Z", (n - 1,)), ("ZZ", (0, 1)), ("XY", (3, 9)), ("ZXXXZ", (5, 6, 7, 8, 9)), ("YY", (n - 2, n - 1)),
            ("XZ", (0, n - 1)), ("Y", (n // 2,)), ("ZXZ", (n - 4, n - 3, n - 2)), ("XX", (7, 8))]


IDENTITY = 1  # of _strings


def _widths(n):
    return [w for w in (1, 4, 9, 10, 17) if w <= n]


class Out:
    """One array of a result: ``axes`` are its state axes (a result involves a canary where one of those indices is one) and
    ``one`` marks the entries the documented contract writes as exactly 1.0 without arithmetic, whatever the state."""

    def __init__(self, a, axes, one=None):
        self.a, self.axes = np.asarray(a), tuple(axes)
        self.one = np.zeros(self.a.shape, dtype=bool) if one is None else np.broadcast_to(one, self.a.shape)

    def involved(self, idx):
        m = np.zeros(self.a.shape, dtype=bool)
        for ax in self.axes:
            sl = [slice(None)] * self.a.ndim
            sl[ax] = list(idx)
            m[tuple(sl)] = True
        return m


def _pair_one(T):
    one = np.zeros(T.shape, dtype=bool)
    one[..., 0, 0] = True  # include/qkgram.h: out2[..][0][0] is exactly 1.0
    return one


def _e_paulis(ctx, d):
    F, nrm = ctx.local_paulis(d, norms=True)
    return [Out(F, [0]), Out(nrm, [0])]


def _e_pairs(dist):
    def run(ctx, d):
        T, F, nrm = ctx.local_pair_paulis(d, singles=True, norms=True, max_dist=dist)
        return [Out(T, [0], _pair_one(T)), Out(F, [0]), Out(nrm, [0])]
    return run


def _e_strings(ctx, d):
    n = d.info()["n_sites"]
    V, nrm = ctx.pauli_expectations(d, _strings(n), norms=True)
    one = np.zeros(V.shape, dtype=bool)
    one[:, IDENTITY] = True  # include/qkgram.h: an all-identity string is written as exactly 1.0
    return [Out(V, [0], one), Out(nrm, [0])]


def _e_purities(ctx, d):
    P, nrm = ctx.bond_purities(d, norms=True)
    return [Out(P, [0]), Out(nrm, [0])]


def _e_block(side):
    def run(ctx, d):
        O, Sx, _ = ctx.block_overlaps(d, None, widths=_widths(d.info()["n_sites"]), side=side)
        return [Out(O, [1, 2]), Out(Sx, [1])]
    return run


def _e_block_self(ctx, d):
    outs = []
    for side in ("left", "right"):
        S, nrm = ctx.block_self(d, widths=_widths(d.info()["n_sites"]), side=side, norms=True)
        outs += [Out(S, [1]), Out(nrm, [0])]
    return outs


ENTRIES = {  # name: (the call, its QK_*_BATCH or None)
    "local_paulis": (_e_paulis, None),
    "local_pair_paulis-1": (_e_pairs(1), None),
    "local_pair_paulis-3": (_e_pairs(3), None),
    "pauli_expectations": (_e_strings, "QK_STRINGS_BATCH"),
    "bond_purities": (_e_purities, None),
    "block_overlaps-left": (_e_block("left"), "QK_BLOCK_BATCH"),
    "block_overlaps-right": (_e_block("right"), "QK_BLOCK_BATCH"),
    "block_self": (_e_block_self, "QK_BLOCK_BATCH"),
}
LOCAL_SETS = {**{f"g20/{k}": ("g20", v) for k, v in H.LOCAL_CANARY_PLACEMENTS.items()}, "g300/0": ("g300", H.LOCAL_CANARIES_300)}


def _twins(which):
    return list((H.gauge_sets if which == "g20" else H.gauge_set_300)()[1])


def _clear_local_env(monkeypatch):
    for k in LOCAL_VARS:
        monkeypatch.delenv(k, raising=False)


def _equal_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("case", list(LOCAL_SETS))
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_local_sweeps_keep_a_canary_to_its_rows(built, monkeypatch, entry, case):
    from qml_cutensornet_amd import engine

    which, idx = LOCAL_SETS[case]
    call, batch_var = ENTRIES[entry]
    twins = _twins(which)
    dirty = H.with_canaries(twins, idx)
    _clear_local_env(monkeypatch)
    with engine.context(0) as ctx, ctx.upload(twins) as dc, ctx.upload(dirty) as dd:
        for cap in (None, "1") if batch_var else (None,):
            if cap:
                monkeypatch.setenv(batch_var, cap)
            ref, got = call(ctx, dc), call(ctx, dd)
            n_nan = n_inv = 0
            for r, g in zip(ref, got):
                assert np.isfinite(r.a).all() and r.a.shape == g.a.shape
                inv = g.involved(idx) & ~g.one
                nan = np.isnan(g.a)
                assert np.array_equal(nan, inv), (entry, case, cap, "NaN entries are not the canary's", np.argwhere(nan != inv)[:8].tolist())
                assert np.array_equal(g.a[~inv], r.a[~inv]), (entry, case, cap, "a clean row differs", float(np.abs(g.a[~inv] - r.a[~inv]).max()))
                assert np.all(g.a[g.one] == 1.0) and np.all(r.a[r.one] == 1.0)
                n_nan, n_inv = n_nan + int(nan.sum()), n_inv + int(inv.sum())
            assert n_nan == n_inv > 0
            again = call(ctx, dc)  # and the clean call after the canaries' is the clean call before it
            assert all(_equal_bits(a.a, r.a) for a, r in zip(again, ref)), (entry, case, cap, "the clean call after the canaries")
            print(f"canary {entry} {case} ({batch_var}={cap}): {n_nan} NaN values = the values of states {list(idx)}; clean rows: bits asserted")


@pytest.mark.parametrize("case", list(LOCAL_SETS))
def test_window_rdms_amplitudes_and_sample_refuse_a_canary(built, monkeypatch, case):
    """A norm that is not finite is refused (QK_EDEVICE), and the message names the first such state."""
    from qml_cutensornet_amd import engine

    which, idx = LOCAL_SETS[case]
    twins = _twins(which)
    n = len(twins[0])
    dirty = H.with_canaries(twins, idx)
    first = rf"state {min(idx)}\b"
    bits = np.random.default_rng(3).integers(0, 2, (5, n), dtype=np.uint8)
    bases = engine.random_bases(5, n, 9)
    _clear_local_env(monkeypatch)
    with engine.context(0) as ctx, ctx.upload(twins) as dc, ctx.upload(dirty) as dd:
        ref = (ctx.window_rdms(dc, 2), ctx.amplitudes(dc, bits, bases=bases, logp=True)[1], ctx.sample(dc, 5, bases=bases, seed=4, logp=True)[1])
        with pytest.raises(engine.QkError, match=first):
            ctx.window_rdms(dd, 2)
        with pytest.raises(engine.QkError, match=first):
            ctx.amplitudes(dd, bits, bases=bases, logp=True)
        with pytest.raises(engine.QkError, match=first):
            ctx.sample(dd, 5, bases=bases, seed=4)
        got = (ctx.window_rdms(dc, 2), ctx.amplitudes(dc, bits, bases=bases, logp=True)[1], ctx.sample(dc, 5, bases=bases, seed=4, logp=True)[1])
    assert all(_equal_bits(g, r) and np.isfinite(r).all() for g, r in zip(got, ref))


# ------------------------------------------------------------------------------------------------------------ (c) a poisoned history
def _all_nan_but_ones(outs):
    return all(np.isnan(o.a[~o.one]).all() and np.all(o.a[o.one] == 1.0) and o.a.size > 0 for o in outs)


def _p_overlaps(ctx, canaries):
    return [Out(ctx.overlaps(canaries), [0, 1])]


POISONERS = {  # NaN-tolerant entry points, run on the all-canary copy of the victim's set (QK_EDGE=4 holds for the whole case)
    "overlaps-edge4": _p_overlaps,  # scratch, derive_tmp, the edge and merged images
    "local_pair_paulis-3": _e_pairs(3),
    "pauli_expectations": _e_strings,
    "block_overlaps": _e_block("left"),
    "bond_purities": _e_purities,
}


def _v_windows(w):
    def run(ctx, d):
        rho, nrm = ctx.window_rdms(d, w, norms=True)
        return [rho, nrm]
    return run


def _v_amplitudes(ctx, d):
    from test_amplitude_host import amp_case

    _, bits, bases = amp_case("g20")
    mant, expo, lp, nrm = ctx.amplitudes(d, bits, bases=bases, per_state=True, scaled=True, logp=True, norms=True)
    return [mant, expo, lp, nrm]


def _v_sample(ctx, d):
    _, bases, seed, _ = H.gauge_sample_case("g20")
    bits, lp = ctx.sample(d, H.SHOTS, bases=bases, seed=seed, logp=True)
    return [bits, lp]


def _v_spectra(ctx, d):
    S, nrm = ctx.bond_spectra(d, norms=True)
    return [S, nrm]


def _v_compress(ctx, d):
    out, info = ctx.compress(d, max_bond=48, info=True)
    try:
        tensors = [t for m in out.download() for t in m.tensors]
    finally:
        out.close()
    return tensors + [info["fidelity"], info["discarded"], info["bond_dims"]]


def _plain(call):
    return lambda ctx, d: [o.a for o in call(ctx, d)]


LOCAL_VICTIMS = {**{name: _plain(call) for name, (call, _) in ENTRIES.items()},
                 "window_rdms-1": _v_windows(1), "window_rdms-2": _v_windows(2), "window_rdms-3": _v_windows(3),
                 "amplitudes": _v_amplitudes, "sample": _v_sample, "bond_spectra": _v_spectra, "compress": _v_compress}


def _history_case(monkeypatch, tag, env, states, victim, upload, bits, kernel=None):
    """``victim(ctx, set)`` -> list of arrays, on a fresh context (r0) and then, on one shared context, around every poisoner and
    around a poisoner followed by Context.trim()."""
    from qml_cutensornet_amd import engine

    _set_env(monkeypatch, dict(env, QK_EDGE="4"))
    _clear_local_env(monkeypatch)
    canaries = H.with_canaries(states, range(len(states)))

    def compare(got, ref, what, eps):
        worst = 0.0
        for g, r in zip(got, ref):
            assert np.isfinite(np.asarray(r, dtype=np.complex128)).all(), (tag, what, "not finite")
            ok, d = _same(np.asarray(g, dtype=np.complex128), np.asarray(r, dtype=np.complex128), bits, eps)
            assert g.shape == r.shape and ok, (tag, what, d)
            worst = max(worst, d)
        assert len(got) == len(ref)
        return worst

    with engine.context(0) as fresh:
        d = upload(fresh, states)
        r0 = victim(fresh, d)
        if kernel:
            assert fresh.stats()["kernel_name"] == kernel, fresh.stats()["kernel_name"]
    worst = 0.0
    with engine.context(0) as ctx:
        d, dc = upload(ctx, states), ctx.upload(canaries)
        for name, poison in list(POISONERS.items()) + [("overlaps-edge4 + trim", _p_overlaps), ("pauli_expectations + trim", _e_strings)]:
            first = victim(ctx, d)  # sizes the buffers
            assert _all_nan_but_ones(poison(ctx, dc)), (tag, name, "the poisoner's own output is not all NaN")
            if name.endswith("trim"):
                ctx.trim()
            third = victim(ctx, d)
            worst = max(worst, compare(third, first, f"after {name}: against the call before", LAUNCH_EPS), compare(third, r0, f"after {name}: against a fresh context", SWEEP_EPS),
                        compare(first, r0, f"before {name}: against a fresh context", SWEEP_EPS))
    print(f"canary history {tag}: {len(POISONERS)} poisoners and 2 with trim(): worst difference {worst:.2e}; {'bits asserted' if bits else 'bounds 1e-13 / 1e-14'}")


@pytest.mark.parametrize("victim", list(LOCAL_VICTIMS))
def test_a_poisoned_history_does_not_reach_a_local_sweep(built, monkeypatch, victim):
    twins = _twins("g20")
    _history_case(monkeypatch, victim, {}, twins, LOCAL_VICTIMS[victim], lambda ctx, s: ctx.upload(s), bits=True)


SWEEP_VICTIMS = {  # name: (set, switches, kernel, bits, complex64 storage) -- the kernels of (a) on "fused8" and "wave2"
    "two-wg/plain": ("fused8", dict(FUSED["two-wg"][1], QK_DETERMINISTIC="0", QK_MERGE="1"), TWO.format(det="false"), False, False),
    "two-wg/det": ("fused8", dict(FUSED["two-wg"][1], QK_DETERMINISTIC="1", QK_MERGE="1"), TWO.format(det="true"), True, False),
    "ring-fused8": ("fused8",) + OTHER["ring-fused8"][1:3] + (False, False),
    "ring-float": ("fused8",) + FLOAT["ring-float"][1:] + (False, True),
    "wave2-ring": ("wave2",) + OTHER["wave2-ring"][1:3] + (False, False),
    "wave2-plain-loads": ("wave2",) + OTHER["wave2-plain-loads"][1:3] + (False, False),
    "wave2-complex64": ("wave2",) + OTHER["wave2-complex64"][1:3] + (False, True),
    "small": ("wave2",) + OTHER["small"][1:3] + (False, False),
    "small-float": ("wave2",) + FLOAT["small-float"][1:] + (False, True),
}


@pytest.mark.parametrize("case", list(SWEEP_VICTIMS))
def test_a_poisoned_history_does_not_reach_a_sweep(built, monkeypatch, case):
    name, env, kernel, bits, f32 = SWEEP_VICTIMS[case]
    xs = _rect_sets(name)[0]

    def victim(ctx, d):
        z = ctx.overlaps(d)
        assert ctx.stats()["kernel_name"] == kernel, ctx.stats()["kernel_name"]
        return [z, ctx.gram(d)]

    _history_case(monkeypatch, case, env, xs, victim, lambda ctx, s: _upload(ctx, s, f32), bits=bits, kernel=kernel)
