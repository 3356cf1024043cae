"""GPU tier: the hand-off from one pair to the next inside a persistent sweep kernel, against the oracle.

Every sweep kernel pulls pairs from a device queue until the queues are empty; the product runs with hundreds of pairs per workgroup,
the rest of the suite with one.  Here every launch holds at least THREE pairs per workgroup (asserted from the stats: pairs >= 3 grid), on
sets whose neighbours in a queue differ in everything the hand-off touches (tests/helpers.py: MANY_PAIR_SETS -- number of tiles, X in LDS
in place / ping-pong / in the global buffer, k-tails of 1..3, a single block, odd column blocks).  Per case:

  1. oracle:    z of the rectangle and K of a symmetric set against oracle/c_oracle.gram_pairs on the same tensors (the suite's TOL), K == K.T;
  2. position:  the same pairs swept again in sub-sets of at most 8 x 8 states, fresh uploads, one pair per workgroup at most (asserted:
                pairs <= grid), entry by entry against the large launch: 1e-13 (the suite's bound between two sweeps of one build), the same
                BITS in the DET forms of the fused kernels.
                QK_EDGE and QK_MERGE are pinned, so that both sides walk the same steps; the rectangular plans have no orientation to
                choose.  A DET value depends on the two states (the step table of their bonds) and on the kernel's shape (the order of
                the turn counters) alone;
  3. duplicates: the first state of every set is also its last one: the four entries of that pair and the two rows agree (bits in DET);
  4. repeat:    a second sweep on the same context and buffers: LAUNCH_EPS, bits in DET (queue heads, turn counters zeroed per launch).

The large launch runs twice over: with the tiled plan (8 queues per class of pairs, both classes in ONE launch of a forced shape: 16 queues,
qk_pull's `((xcc + s) & 7) + (s & 8)`) and with the flat list of Context.overlaps (one queue).  Further cases: the two launches of a split
sweep and of a mixed set (a second run of >= 1536 / >= 6144 pairs), and the three shares of a 3-rank plan.

The LDS-resident small-bond sweep takes bonds <= 32 only, so it runs on the wave2 set; the ring sweep takes both fused sets."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

TOL = 1e-11         # against the oracle (the suite's)
SWEEP_EPS = 1e-13   # between two sweeps of one build (the suite's)
LAUNCH_EPS = 1e-14  # between two launches on the same buffers (the suite's)
CHUNK = 8

QK_VARS = ("QK_FUSED_WGS", "QK_FUSED_DUAL", "QK_FUSED", "QK_FUSED_SPLIT", "QK_EDGE", "QK_MERGE", "QK_DETERMINISTIC", "QK_WAVE", "QK_WAVE2", "QK_SMALL",
           "QK_WGS_PER_CU", "QK_PLAN_NO_MIXED", "QK_PLAN_ORIENT", "QK_GANG")
DUAL = "qk_sweep_fused_dual_kernel<12, 8192, 3, {det}>"
ONE = "qk_sweep_fused_kernel<12, 2, 8192, 3, {det}>"
TWO = "qk_sweep_fused_kernel<8, 1, 4608, 4, {det}>"
FUSED = {  # shape: (set, switches, kernel).  QK_PLAN_NO_MIXED: the symmetric sets hold enough small states for a second run on the one-wave sweep, which has a case of its own
    "dual": ("fused12", {"QK_FUSED_WGS": "1", "QK_FUSED_DUAL": "1", "QK_PLAN_NO_MIXED": "1"}, DUAL),
    "one-tile": ("fused12", {"QK_FUSED_WGS": "1", "QK_FUSED_DUAL": "0", "QK_PLAN_NO_MIXED": "1"}, ONE),
    "two-wg": ("fused8", {"QK_FUSED_WGS": "2", "QK_PLAN_NO_MIXED": "1"}, TWO),
}
CHAINS = {"plain-chain": {"QK_EDGE": "0", "QK_MERGE": "0"}, "edge4-merged": {"QK_EDGE": "4", "QK_MERGE": "1"}}
NOT_WAVE = {"QK_WAVE": "0", "QK_WAVE2": "0", "QK_WGS_PER_CU": "1"}  # (the switches of test_small_bond_kernel)
OTHER = {  # case: (set, switches, kernel, queues of the tiled plan's launch, complex64 storage)
    "wave2-ring": ("wave2", {}, "qk_sweep_wave2_kernel<3, double>", 8, False),
    "wave2-plain-loads": ("wave2", {"QK_WAVE2": "2"}, "qk_sweep_wave2_kernel<0, double>", 8, False),
    "wave2-complex64": ("wave2", {}, "qk_sweep_wave2_kernel<3, float>", 8, True),
    "wave": ("wave", {}, "qk_sweep_wave_kernel<0>", 1, False),
    "small": ("wave2", NOT_WAVE, "qk_sweep_small_kernel<double>", 1, False),
    "ring-fused8": ("fused8", dict(NOT_WAVE, QK_SMALL="0", QK_FUSED="0"), "qk_sweep_ring_kernel<double>", 1, False),
    "ring-fused12": ("fused12", dict(NOT_WAVE, QK_SMALL="0", QK_FUSED="0"), "qk_sweep_ring_kernel<double>", 1, False),
}

_refs = {}


def _tensors(states, f32):
    if f32:  # complex64 storage: the sweep is the fp64 sweep of the rounded tensors
        return [[t.astype(np.complex64).astype(np.complex128) for t in m.tensors] for m in states]
    return [m.tensors for m in states]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _rect_ref(name, f32=False):
    """(xs, ys, sym, z_ref[ny, nx], K_ref) of a rectangular set: made once for the module, read-only."""
    from oracle import c_oracle

    if (name, f32) not in _refs:
        xs, ys = _refs[(name, False)][:2] if (name, False) in _refs else H.many_pair_sets(name)
        sym = H.many_pair_symmetric(name, xs, ys)
        nx, ny, ns = len(xs), len(ys), len(sym)
        pr = np.array([(i, j) for j in range(ny) for i in range(nx)], dtype=np.int32)
        _, z, _ = c_oracle.gram_pairs(_tensors(xs, f32), _tensors(ys, f32), pr, 8)
        ps = np.array([(i, j) for j in range(ns) for i in range(j + 1)], dtype=np.int32)
        v, _, _ = c_oracle.gram_pairs(_tensors(sym, f32), None, ps, 8)
        K = np.zeros((ns, ns))
        K[ps[:, 1], ps[:, 0]] = v
        K[ps[:, 0], ps[:, 1]] = v
        _refs[(name, f32)] = (xs, ys, sym) + _frozen(z.reshape(ny, nx), K)
    return _refs[(name, f32)]


def _gram_ref(name):
    """(xs, pairs -> z of the oracle, K_ref) of a symmetric set."""
    from oracle import c_oracle

    if name not in _refs:
        xs = H.many_pair_gram_set(name)
        ns = len(xs)
        ps = np.array([(i, j) for j in range(ns) for i in range(ns)], dtype=np.int32)
        v, z, _ = c_oracle.gram_pairs([m.tensors for m in xs], None, ps, 8)
        _refs[name] = (xs,) + _frozen(z.reshape(ns, ns), v.reshape(ns, ns))  # z[j, i] = <x_i|x_j>
    return _refs[name]


def _set_env(monkeypatch, env):
    for k in QK_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _same(a, b, bits, eps):
    """(ok, worst difference): the same bits, or within eps."""
    d = float(np.abs(np.asarray(a) - np.asarray(b)).max())
    return (np.array_equal(a, b) if bits else d < eps), d


def _upload(ctx, states, f32):
    d = ctx.upload(states)
    if not f32:
        return d
    f = d.to_f32()
    d.close()
    return f


def _sweep_plan(ctx, dx, dy, plan):
    """z[j, i] of a plan's pairs (NaN where the plan has none) and the stats of the launch."""
    _, z = ctx.gram_values_host(dx, dy, plan, want_z=True)
    pr = plan.pairs()
    out = np.full((len(dx) if dy is None else len(dy), len(dx)), np.nan + 0j)
    assert len(np.unique(pr[:, 1].astype(np.int64) * len(dx) + pr[:, 0])) == len(pr)
    out[pr[:, 1], pr[:, 0]] = z
    return out, ctx.stats()


def _check_duplicates(z, bits, what):
    """The first state of the x set (columns) and of the y set (rows) is also the last one."""
    four = [z[0, 0], z[0, -1], z[-1, 0], z[-1, -1]]
    ok, d = _same(four, [four[0]] * 4, bits, SWEEP_EPS)
    assert ok, (what, "the duplicated pair", four)
    ok, d = _same(z[0], z[-1], bits, SWEEP_EPS)
    assert ok, (what, "the duplicated y state", d)
    ok, d = _same(z[:, 0], z[:, -1], bits, SWEEP_EPS)
    assert ok, (what, "the duplicated x state", d)


def _many_pairs_case(monkeypatch, tag, name, env, kernel, queues, bits, f32=False):
    from qml_cutensornet_amd import engine

    xs, ys, sym, z_ref, K_ref = _rect_ref(name, f32)
    nx, ny = len(xs), len(ys)
    _set_env(monkeypatch, env)
    with engine.context(0) as ctx:
        dx, dy, ds = _upload(ctx, xs, f32), _upload(ctx, ys, f32), _upload(ctx, sym, f32)
        plan = engine.Plan(dx.dims, dy.dims)
        assert plan.num_pairs == nx * ny
        z, st = _sweep_plan(ctx, dx, dy, plan)
        assert st["kernel_name"] == kernel and st["second_kernel"] == 0, (st["kernel_name"], st["second_kernel_name"])
        assert st["pairs"] == nx * ny and st["pairs"] >= 3 * st["grid"] > 0 and st["queues"] == queues, st
        z_again, _ = _sweep_plan(ctx, dx, dy, plan)  # 4: the same context, sets, plan
        plan.close()
        z_flat = ctx.overlaps(dx, dy)  # the flat list: one queue
        st_flat = ctx.stats()
        assert st_flat["kernel_name"] == kernel and st_flat["pairs"] >= 3 * st_flat["grid"] > 0 and st_flat["queues"] == 1, st_flat
        K = ctx.gram(ds)
        st_sym = ctx.stats()
        assert st_sym["kernel_name"] == kernel and st_sym["second_kernel"] == 0 and st_sym["pairs"] >= 3 * st_sym["grid"] > 0, st_sym
        K_again = ctx.gram(ds)
    # 2: one pair per workgroup at most
    z_one = np.full((ny, nx), np.nan + 0j)
    with engine.context(0) as ctx:
        for j0 in range(0, ny, CHUNK):
            for i0 in range(0, nx, CHUNK):
                cx, cy = _upload(ctx, xs[i0:i0 + CHUNK], f32), _upload(ctx, ys[j0:j0 + CHUNK], f32)
                sub = engine.Plan(cx.dims, cy.dims)
                z_one[j0:j0 + CHUNK, i0:i0 + CHUNK], st1 = _sweep_plan(ctx, cx, cy, sub)
                assert st1["kernel_name"] == kernel and 0 < st1["pairs"] <= st1["grid"], (i0, j0, st1)
                sub.close(), cx.close(), cy.close()
    e_ref, e_flat, e_K = float(np.abs(z - z_ref).max()), float(np.abs(z_flat - z_ref).max()), float(np.abs(K - K_ref).max())
    ok_one, d_one = _same(z, z_one, bits, SWEEP_EPS)
    ok_flat, d_flat = _same(z, z_flat, bits, SWEEP_EPS)
    ok_rep, d_rep = _same(z, z_again, bits, LAUNCH_EPS)
    ok_repK, d_repK = _same(K, K_again, bits, LAUNCH_EPS)
    print(f"many-pairs {tag}: {kernel}: grid {st['grid']}, pairs {st['pairs']}, queues {st['queues']} (symmetric: grid {st_sym['grid']}, pairs {st_sym['pairs']}); "
          f"max |z - oracle| {e_ref:.2e} (flat list {e_flat:.2e}), |K - oracle| {e_K:.2e}; many pairs against one pair per workgroup {d_one:.2e}, against the flat list "
          f"{d_flat:.2e}; second launch {d_rep:.2e} (K {d_repK:.2e}); {'bits asserted' if bits else 'bounds 1e-13 / 1e-14'}")
    assert e_ref < TOL and e_flat < TOL and e_K < TOL
    assert np.array_equal(K, K.T)
    assert ok_one, ("many pairs per workgroup against one", d_one, np.argwhere(z != z_one)[:8].tolist())
    assert ok_flat, ("tiled plan against the flat list", d_flat)
    assert ok_rep and ok_repK, ("second launch", d_rep, d_repK)
    _check_duplicates(z, bits, "z")
    m = nx - 1  # the symmetric set begins with xs: state m is state 0
    four = [K[0, 0], K[0, m], K[m, 0], K[m, m]]
    assert _same(four, [four[0]] * 4, bits, SWEEP_EPS)[0], four
    assert np.abs(K[0] - K[m]).max() < SWEEP_EPS and np.abs(K[:, 0] - K[:, m]).max() < SWEEP_EPS  # (an oriented plan may turn one of the two)


@pytest.mark.parametrize("chain", list(CHAINS))
@pytest.mark.parametrize("det", [False, True], ids=["plain", "det"])
@pytest.mark.parametrize("shape", list(FUSED))
def test_fused_sweeps_hand_pairs_on(built, monkeypatch, shape, det, chain):
    name, env, kernel = FUSED[shape]
    env = dict(env, QK_DETERMINISTIC="1" if det else "0", **CHAINS[chain])
    _many_pairs_case(monkeypatch, f"{shape}/{chain}", name, env, kernel.format(det="true" if det else "false"), 8, bits=det)


@pytest.mark.parametrize("case", list(OTHER))
def test_one_wave_small_and_ring_sweeps_hand_pairs_on(built, monkeypatch, case):
    name, env, kernel, queues, f32 = OTHER[case]
    _many_pairs_case(monkeypatch, case, name, env, kernel, queues, bits=False, f32=f32)


def _two_launch_case(monkeypatch, tag, name, env, kernels, min_first, min_second, bits):
    """Checks 1, 3 and 4 on a symmetric Gram whose plan has two runs, each a launch of its own."""
    from qml_cutensornet_amd import engine

    xs, z_ref, K_ref = _gram_ref(name)
    ns = len(xs)
    _set_env(monkeypatch, env)
    with engine.context(0) as ctx, ctx.upload(xs) as dx:
        plan = engine.Plan(dx.dims)
        first, second = plan.first_run, plan.num_pairs - plan.first_run
        assert first >= min_first and second >= min_second, (first, second)
        z, st = _sweep_plan(ctx, dx, None, plan)
        firsts = kernels[0] if isinstance(kernels[0], tuple) else (kernels[0],)
        assert st["kernel_name"] in firsts and st["second_kernel_name"] == kernels[1], (st["kernel_name"], st["second_kernel_name"])
        kernels = (st["kernel_name"], kernels[1])  # every further launch: the same two
        assert st["queues"] == 8 and st["second_pairs"] == second and st["pairs"] == first + second and st["pairs"] >= 3 * st["grid"] > 0, st
        z_again, _ = _sweep_plan(ctx, dx, None, plan)
        plan.close()
        K = ctx.gram(dx)
        st_K = ctx.stats()
        assert (st_K["kernel_name"], st_K["second_kernel_name"]) == kernels and st_K["second_pairs"] == second
        K_again = ctx.gram(dx)
    have = ~np.isnan(z)  # an oriented plan lists (i, j) or (j, i)
    assert np.all(have | have.T) and have.sum() == first + second
    e_ref, e_K = float(np.abs(z[have] - z_ref[have]).max()), float(np.abs(K - K_ref).max())
    ok_rep, d_rep = _same(z[have], z_again[have], bits, LAUNCH_EPS)
    ok_repK, d_repK = _same(K, K_again, bits, LAUNCH_EPS)
    print(f"many-pairs {tag}: {kernels[0]} + {kernels[1]}: grid {st['grid']}, pairs {first} + {second}, queues {st['queues']}; max |z - oracle| {e_ref:.2e}, "
          f"|K - oracle| {e_K:.2e}; second sweep {d_rep:.2e} (K {d_repK:.2e}); {'bits asserted' if bits else 'bound 1e-14'}")
    assert e_ref < TOL and e_K < TOL and np.array_equal(K, K.T)
    assert ok_rep and ok_repK, (d_rep, d_repK)
    m = ns - 1  # state m is state 0
    four = [K[0, 0], K[0, m], K[m, 0], K[m, m]]
    assert _same(four, [four[0]] * 4, bits, SWEEP_EPS)[0], four
    assert np.abs(K[0] - K[m]).max() < SWEEP_EPS and np.abs(K[:, 0] - K[:, m]).max() < SWEEP_EPS
    zz = np.where(have, z, np.conj(z.T))  # <x_i|x_j> whichever way round the plan lists it
    assert np.abs(zz[0] - zz[m]).max() < SWEEP_EPS and np.abs(zz[:, 0] - zz[:, m]).max() < SWEEP_EPS


@pytest.mark.parametrize("det", [False, True], ids=["plain", "det"])
def test_split_sweep_two_launches_of_many_pairs(built, monkeypatch, det):
    d = "true" if det else "false"
    _two_launch_case(monkeypatch, "split", "split", {"QK_FUSED_SPLIT": "2", "QK_DETERMINISTIC": "1" if det else "0"}, (DUAL.format(det=d), TWO.format(det=d)), 768, 1536, bits=det)


@pytest.mark.parametrize("det", [False, True], ids=["plain", "det"])
def test_mixed_set_second_launch_of_many_small_pairs(built, monkeypatch, det):
    d = "true" if det else "false"  # (which fused shape takes the first run is the planner's business)
    _two_launch_case(monkeypatch, "mixed", "mixed", {"QK_DETERMINISTIC": "1" if det else "0"}, ((DUAL.format(det=d), TWO.format(det=d)), "qk_sweep_wave2_kernel<3, double>"),
                     1, 6144, bits=det)


@pytest.mark.parametrize("det", [False, True], ids=["plain", "det"])
def test_rank_shares_of_many_pairs_reassemble(built, monkeypatch, det):
    from qml_cutensornet_amd import engine

    xs, ys, _, z_ref, _ = _rect_ref("fused12-ranks")
    nx, ny, world = len(xs), len(ys), 3
    kernel = DUAL.format(det="true" if det else "false")
    _set_env(monkeypatch, dict(FUSED["dual"][1], QK_DETERMINISTIC="1" if det else "0", **CHAINS["edge4-merged"]))
    with engine.context(0) as ctx, ctx.upload(xs) as dx, ctx.upload(ys) as dy:
        whole = engine.Plan(dx.dims, dy.dims)
        z, st = _sweep_plan(ctx, dx, dy, whole)
        assert st["kernel_name"] == kernel and st["pairs"] == nx * ny
        whole.close()
        z_shares = np.full((ny, nx), np.nan + 0j)
        sizes = []
        for r in range(world):
            share = engine.Plan(dx.dims, dy.dims, world, r)
            zr, sr = _sweep_plan(ctx, dx, dy, share)
            assert sr["kernel_name"] == kernel and sr["pairs"] == share.num_pairs and sr["pairs"] >= 3 * sr["grid"] > 0, sr
            mine = ~np.isnan(zr)
            assert not np.any(mine & ~np.isnan(z_shares))  # no pair twice
            z_shares[mine] = zr[mine]
            sizes.append((sr["grid"], sr["pairs"]))
            share.close()
    assert not np.isnan(z_shares).any()
    ok, d = _same(z, z_shares, det, SWEEP_EPS)
    e_ref = float(np.abs(z_shares - z_ref).max())
    print(f"many-pairs ranks: {kernel}: (grid, pairs) of the shares {sizes}; max |z - oracle| {e_ref:.2e}; shares against one rank {d:.2e}; {'bits asserted' if det else 'bound 1e-13'}")
    assert e_ref < TOL and float(np.abs(z - z_ref).max()) < TOL
    assert ok, d
