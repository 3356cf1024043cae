"""CPU tier of tests/test_gpu_canary.py: the conditions the canary tests rest on, checked without a GPU.

A canary state (tests/helpers.py: canary_copy) has the bond table of a clean state and NaN in every tensor element.  The GPU tests
take for granted that (1) a set with canaries has the dims table of the clean set, so that engine.Plan -- which sees dims alone -- is
the same pairs in the same order in the same queues, for one rank and for the shares of three; (2) the canaries are between 30 % and
55 % of the pairs of every case, include a state of the set's largest cap and leave the duplicated first and last states alone; (3)
"a result involves a canary" means what the host mirrors say: NaN for a pair, a feature, a window of a canary, the same bits as
before for everything else."""
import numpy as np
import pytest

import helpers as H

RECT = list(H.MANY_PAIR_SETS)
GRAMS = list(H.MANY_PAIR_GRAMS)


def _rect_dims(name):
    n = H.MANY_PAIR_SETS[name][0]
    cx, cy = H.many_pair_caps(name)
    return H.capped_dims(n, cx), H.capped_dims(n, cy)


def _same_plan(a, b):
    assert a.num_pairs == b.num_pairs and a.first_run == b.first_run
    assert np.array_equal(a.pairs(), b.pairs())
    (na, qa), (nb, qb) = a.queues(), b.queues()
    assert na == nb and np.array_equal(qa, qb)


def test_canary_copy_keeps_the_shapes_and_poisons_every_element(built):
    xs, _ = H.many_pair_sets("wave")
    m = xs[3]
    c = H.canary_copy(m)
    assert np.array_equal(c.bond_dims(), m.bond_dims()) and len(c) == len(m)
    for t, u in zip(m.tensors, c.tensors):
        assert u.shape == t.shape and u.dtype == np.complex128 and np.isnan(u.real).all() and np.isnan(u.imag).all()
        assert np.isfinite(t).all()  # the original is untouched
    idx = H.many_pair_canaries("wave")[0]
    ys = H.with_canaries(xs, idx)
    assert len(ys) == len(xs) and all((ys[i] is xs[i]) == (i not in idx) for i in range(len(xs)))
    assert np.array_equal(np.array([m.bond_dims() for m in ys]), np.array([m.bond_dims() for m in xs]))


def test_canary_indices_rule():
    caps = [5, 9, 7, 9, 3, 5, 8, 7, 2, 5]
    assert H.canary_indices(10, caps, 5) == [1, 2, 7]          # i % 5 == 2, and the first inner 9 (none of 2, 7 has it)
    assert H.canary_indices(10, caps, 3, 1) == [1, 4, 7]       # 1 has the 9 already
    assert H.canary_indices(10, [9] + caps[1:-1] + [9], 5) == [1, 2, 7]  # never the first or the last state
    assert H.canary_indices(13, list(range(12)) + [0], 5) == [2, 7, 11]  # 12 % 5 == 2 is the last state: left out; the largest cap is state 11's


@pytest.mark.parametrize("name", RECT)
def test_rectangular_canary_sets(built, name):
    """Dims, plans, share, largest cap, clean duplicates -- for the rectangle and for the symmetric set made from it."""
    from qml_cutensornet_amd import engine

    xd, yd = _rect_dims(name)
    cx, cy = H.many_pair_caps(name)
    ix, iy = H.many_pair_canaries(name)
    nx, ny = len(cx), len(cy)
    assert ix == [i for i in range(1, nx - 1) if i % 5 == 2] and iy == [j for j in range(1, ny - 1) if j % 3 == 1]  # no state had to be added
    assert 0 not in ix and nx - 1 not in ix and 0 not in iy and ny - 1 not in iy
    assert max(cx[i] for i in ix) == max(cx) and max(cy[j] for j in iy) == max(cy)
    assert {cy[j] for j in iy} == set(cy)  # period 3 reaches every y cap
    mask = H.canary_pair_mask(nx, ix, ny, iy)
    share = mask.mean()
    assert 0.30 <= share <= 0.55, share
    assert 0.46 <= round(share, 2) <= 0.47, share  # (the figure the placement was chosen by)
    if name in ("fused8", "wave"):  # the states themselves: the canary sets have the dims tables of the clean sets
        xs, ys = H.many_pair_sets(name)
        xc, yc = H.with_canaries(xs, ix), H.with_canaries(ys, iy)
        assert np.array_equal(np.array([m.bond_dims() for m in xc]), xd) and np.array_equal(np.array([m.bond_dims() for m in yc]), yd)
        assert xc[0] is xs[0] and xc[-1] is xs[0] and yc[0] is ys[0] and yc[-1] is ys[0]
        clean, dirty = engine.Plan(engine._dims_table(xs), engine._dims_table(ys)), engine.Plan(engine._dims_table(xc), engine._dims_table(yc))
        _same_plan(clean, dirty)
        clean.close(), dirty.close()
    # the symmetric set: xs and the first states of ys
    isym = H.many_pair_symmetric_canaries(name)
    ns = len(H.many_pair_symmetric(name, list(range(nx)), list(range(ny))))
    assert all(0 < i < ns for i in isym) and nx - 1 not in isym and nx not in isym  # state nx - 1 is state 0; state nx is ys[0]
    sm = H.canary_pair_mask(ns, isym)
    assert np.array_equal(sm, sm.T)
    tri = sm[np.tril_indices(ns)].mean()
    assert 0.30 <= tri <= 0.55, tri
    caps_sym = (cx + cy)[:ns]
    assert max(caps_sym[i] for i in isym) == max(caps_sym)


@pytest.mark.parametrize("name", GRAMS)
def test_gram_canary_sets(built, name):
    caps = H.many_pair_gram_caps(name)
    ns = len(caps)
    idx = H.many_pair_gram_canaries(name)
    period = [i for i in range(1, ns - 1) if i % 5 == 2]
    assert set(period) < set(idx) and len(idx) == len(period) + 1  # period 5 misses the largest cap: one state is added
    assert max(caps[i] for i in period) < max(caps) == max(caps[i] for i in idx)
    assert 0 not in idx and ns - 1 not in idx
    tri = np.tril_indices(ns)
    before = H.canary_pair_mask(ns, period)[tri].mean()
    assert round(before, 3) == {"split": 0.345, "mixed": 0.359}[name], before
    share = H.canary_pair_mask(ns, idx)[tri].mean()
    assert 0.30 <= share <= 0.55, share


def test_rank_shares_do_not_see_the_canaries(built):
    """world_size = 3: a share is made from the dims tables; those of the canary sets are those of the clean sets."""
    from qml_cutensornet_amd import engine

    xs, ys = H.many_pair_sets("fused8")  # (real states: the tables as Context.upload makes them)
    ix, iy = H.many_pair_canaries("fused8")
    dx, dy = engine._dims_table(xs), engine._dims_table(ys)
    cx, cy = engine._dims_table(H.with_canaries(xs, ix)), engine._dims_table(H.with_canaries(ys, iy))
    assert np.array_equal(dx, cx) and np.array_equal(dy, cy)
    xd, yd = _rect_dims("fused12-ranks")
    ix, iy = H.many_pair_canaries("fused12-ranks")
    mask = H.canary_pair_mask(len(xd), ix, len(yd), iy)
    for r in range(3):
        a, b = engine.Plan(xd, yd, 3, r), engine.Plan(xd.copy(), yd.copy(), 3, r)
        _same_plan(a, b)
        pr = a.pairs()
        share = mask[pr[:, 1], pr[:, 0]].mean()
        assert 0.30 <= share <= 0.55, (r, share)  # every share holds its part of the canary pairs
        a.close(), b.close()


LOCAL = (1, 4)


def _padded(t, p=16):
    l, _, r = t.shape
    out = np.zeros(((l + p - 1) // p * p, 2, (r + p - 1) // p * p), dtype=np.complex128)
    out[:l, :, :r] = t
    return out


def _persistent_sweep(pairs, sloppy):
    """A numpy model of a persistent workgroup: ONE X buffer for all its pairs, site tensors zero-padded to 16, every product over
    the padded bond.  The sound form sets the whole first block of X; the ``sloppy`` one sets X[0][0] alone and leaves the rest of
    the block as the previous pair left it -- "the other operand's padding is zero" then has to do the job."""
    buf = np.zeros((128, 128), dtype=np.complex128)
    out = []
    with np.errstate(invalid="ignore"):
        for x, y in pairs:
            if not sloppy:
                buf[:16, :16] = 0.0
            buf[0, 0] = 1.0
            a = b = 16
            for tx, ty in zip(x.tensors, y.tensors):
                A, B = _padded(np.asarray(tx)), _padded(np.asarray(ty))
                X = np.einsum("ab,asc,bsd->cd", buf[:a, :b], A.conj(), B)
                a, b = X.shape
                buf[:a, :b] = X
            out.append(complex(buf[0, 0]))
    return np.array(out)


def test_a_canary_shows_the_stale_read_that_finite_data_hides(built):
    """Why the probe is a NaN: a stale value times a zero pad is 0 while it is finite, so finite data cannot see the read."""
    from oracle import restatement as R

    xs, ys = H.many_pair_sets("wave")
    clean = [(xs[1], ys[2]), (xs[3], ys[1]), (xs[5], ys[5]), (xs[4], ys[3])]
    ref = np.array([R.mps_inner(x.tensors, y.tensors) for x, y in clean])
    assert np.abs(_persistent_sweep(clean, False) - ref).max() < 1e-14
    assert np.array_equal(_persistent_sweep(clean, True), _persistent_sweep(clean, False))  # finite leftovers: the sloppy form passes every test
    dirty = clean[:2] + [(H.canary_copy(xs[2]), ys[4])] + clean[2:]
    sound, sloppy = _persistent_sweep(dirty, False), _persistent_sweep(dirty, True)
    assert np.isnan(sound[2]) and np.array_equal(np.delete(sound, 2), _persistent_sweep(clean, False))  # the canary spoils its own pair
    assert np.isnan(sloppy[2]) and not np.isnan(sloppy[:2]).any() and np.isnan(sloppy[3:]).all()       # ... and here every pair after it


def _local_sets():
    twins = list(H.gauge_sets()[1])
    return twins, H.with_canaries(twins, LOCAL)


def test_local_canary_placements(built):
    """States 1 and 4 of the six twins; a placement of its own holds the profile that reaches 128 (state 3); one of the two of 300."""
    twins = list(H.gauge_sets()[1])
    assert H.LOCAL_CANARY_PLACEMENTS["1-4"] == LOCAL
    reach = {i for idx in H.LOCAL_CANARY_PLACEMENTS.values() for i in idx}
    assert max(twins[i].max_bond() for i in reach) == max(m.max_bond() for m in twins) == 128
    for idx in H.LOCAL_CANARY_PLACEMENTS.values():
        dirty = H.with_canaries(twins, idx)
        assert 0 < len(idx) < len(twins) and np.array_equal(np.array([m.bond_dims() for m in dirty]), np.array([m.bond_dims() for m in twins]))
    big = list(H.gauge_set_300()[1])
    big_dirty = H.with_canaries(big, H.LOCAL_CANARIES_300)
    assert H.LOCAL_CANARIES_300 == (0,) and big_dirty[1] is big[1] and big_dirty[0].max_bond() == 300 and np.isnan(big_dirty[0].tensors[9]).all()


def test_host_mirrors_nan_for_a_canary_bits_for_the_rest(built):
    """What "involves a canary" means for pairs (mps_inner), features (environments) and windows (window_rdm, block_overlap)."""
    from oracle import restatement as R

    xs, ys = H.many_pair_sets("wave")
    ix, iy = H.many_pair_canaries("wave")
    xc, yc = H.with_canaries(xs, ix), H.with_canaries(ys, iy)
    for i in (0, 1, ix[0], ix[0] + 1):
        for j in (0, iy[0], iy[0] + 1):
            z, zc = R.mps_inner(xs[i].tensors, ys[j].tensors), R.mps_inner(xc[i].tensors, yc[j].tensors)
            if i in ix or j in iy:
                assert np.isnan(zc.real) and np.isnan(zc.imag) and np.isfinite(z)
            else:
                assert zc == z and np.isfinite(z)
    twins, dirty = _local_sets()
    with np.errstate(invalid="ignore"):
        for s in (0, 1, 4, 5):
            L, Rr = H.environments(dirty[s].tensors)
            L0, R0 = H.environments(twins[s].tensors)
            if s in LOCAL:  # every environment but the two trivial ones, and the norm
                assert all(np.isnan(m).all() for m in L[1:]) and all(np.isnan(m).all() for m in Rr[:-1])
            else:
                assert all(np.array_equal(a, b) for a, b in zip(L + Rr, L0 + R0))
        for s in (0, 4):
            for w, a in ((1, 0), (2, 7), (3, 17)):
                rho, rho0 = dirty[s].window_rdm(a, w), twins[s].window_rdm(a, w)
                assert np.isnan(rho).all() if s in LOCAL else np.array_equal(rho, rho0)
        for side in ("left", "right"):
            for i, j in ((0, 2), (0, 1), (4, 2), (4, 4), (3, 3)):
                o, o0 = dirty[i].block_overlap(dirty[j], 5, side), twins[i].block_overlap(twins[j], 5, side)
                assert np.isnan(o) if (i in LOCAL or j in LOCAL) else (o == o0 and np.isfinite(o))
