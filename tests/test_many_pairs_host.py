"""CPU tier of tests/test_gpu_many_pairs.py: the sets of tests/helpers.py are what the GPU tests take them for -- long enough for three pairs
per workgroup on a 256-CU part, split where the two-launch cases need it, mixed in the classes the hand-off cares about -- and the C oracle
they are checked against agrees with the restatement."""
import numpy as np
import pytest

import helpers as H

NUM_CUS = 256
XCAP_ONE = 8192  # elements of the 12-wave shapes' LDS X buffer (qk_plan.h)
GRID = {"fused12": 1 * NUM_CUS, "fused12-ranks": 1 * NUM_CUS, "fused8": 2 * NUM_CUS, "wave2": 8 * NUM_CUS, "wave": 16 * NUM_CUS}  # qk_choose_sweep: wgs x num_cus


def _pad(v):
    return (np.asarray(v) + 15) // 16 * 16


def _dims(name):
    n = H.MANY_PAIR_SETS[name][0]
    cx, cy = H.many_pair_caps(name)
    return H.capped_dims(n, cx), H.capped_dims(n, cy)


@pytest.mark.parametrize("name", list(H.MANY_PAIR_SETS))
def test_rectangles_hold_three_pairs_per_workgroup(built, name):
    from qml_cutensornet_amd import engine

    xd, yd = _dims(name)
    plan = engine.Plan(xd, yd)
    pr = plan.pairs()
    assert plan.num_pairs == len(xd) * len(yd) >= 3 * GRID[name]
    assert len({(i, j) for i, j in pr.tolist()}) == len(pr)
    nq, qs = plan.queues()
    assert nq == 16 and qs[0] == 0 and qs[16] == len(pr) and np.all(np.diff(qs) >= 0)
    plan.close()
    ns = len(H.many_pair_symmetric(name, list(range(len(xd))), list(range(len(yd)))))
    assert ns * (ns + 1) // 2 >= 3 * GRID[name]
    # the sub-sets of the position check: one pair per workgroup at most, and the same kernel as the whole set (bonds above 32 / 16 in every chunk)
    big = max(xd.max(), yd.max())
    for i0 in range(0, len(xd), 8):
        assert 8 * 8 <= GRID[name] and (xd[i0:i0 + 8].max() > 32) == (big > 32) and (xd[i0:i0 + 8].max() > 16) == (big > 16)


def test_constructors_make_the_chains_the_planner_is_asked_about(built):
    for name in ("fused8", "wave"):
        xs, ys = H.many_pair_sets(name)
        xd, yd = _dims(name)
        assert np.array_equal(np.array([m.bond_dims() for m in xs]), xd) and np.array_equal(np.array([m.bond_dims() for m in ys]), yd)
        assert xs[-1] is xs[0] and ys[-1] is ys[0] and not any(a is b for a in xs[:-1] for b in ys)


def test_cap_classes_of_the_12_wave_set(built):
    """What the docstring of MANY_PAIR_SETS promises, read from the bond tables and from the plan's pair list."""
    from qml_cutensornet_amd import engine

    xd, yd = _dims("fused12")
    xb, yb = xd.max(axis=1), yd.max(axis=1)
    assert {1, 2, 3} <= {int((b % 16 + 3) // 4) for b in xb if b % 16}  # k-steps in the last block of rows of A below a true bond
    assert 3 in xb and {1, 3, 5, 7} <= {int(_pad(b) // 16) for b in yb}  # a single block; odd numbers of column blocks of B
    plan = engine.Plan(xd, yd)
    pr = plan.pairs()
    nq, qs = plan.queues()
    A, B = _pad(xd[pr[:, 0]]), _pad(yd[pr[:, 1]])
    x_in, x_out = A[:, :-1] * B[:, :-1], A[:, 1:] * B[:, 1:]  # elements of X and X' per site
    glob = ((x_in > XCAP_ONE) | (x_out > XCAP_ONE)).any(axis=1)      # a site above the LDS buffer: X in the global buffer, strips
    in_place = ((x_in <= XCAP_ONE) & (x_out <= XCAP_ONE) & (x_in + x_out > XCAP_ONE)).any(axis=1)
    one_tile = (A.max(axis=1) <= 16) & (B.max(axis=1) <= 16)
    tiles = (A // 16 * (B // 16)).max(axis=1)
    assert glob.sum() >= 100 and in_place.sum() >= 100 and one_tile.sum() >= 16 and (~glob & ~in_place).sum() >= 100
    # The planner puts the pairs whose work fits the smaller buffer into a class of their own (queues 8..15), so a global-X pair and a one-tile pair
    # never share a queue: a workgroup of the one launch goes from the first class's queues to the second's when the first are empty, which is where
    # the largest pairs are followed by the smallest.  Inside a queue: a global-X pair directly followed by an LDS-resident one, and the reverse.
    first = plan.first_run
    assert qs[8] == first and glob[:first].any() and not glob[first:].any() and one_tile[first:].any() and not one_tile[:first].any()
    down = up = 0
    for s in range(nq):
        t = np.arange(qs[s], qs[s + 1] - 1)
        down += int((glob[t] & ~glob[t + 1]).sum())
        up += int((~glob[t] & glob[t + 1]).sum())
        assert qs[s + 1] - qs[s] >= 16 and len(set(tiles[qs[s]:qs[s + 1]].tolist())) >= 2, s  # no queue holds one size of pair only
    assert down >= 1 and up >= 1
    plan.close()


def test_two_launch_sets_split_where_the_cases_need_it(built):
    from qml_cutensornet_amd import engine

    n, _, _ = H.MANY_PAIR_GRAMS["split"]
    plan = engine.Plan(H.capped_dims(n, H.many_pair_gram_caps("split")))
    assert plan.first_run >= 3 * NUM_CUS and plan.num_pairs - plan.first_run >= 3 * 2 * NUM_CUS  # 768 for the 12-wave shape, 1536 for two workgroups per CU
    assert plan.stats()["pairs"] == plan.num_pairs
    plan.close()
    n, _, _ = H.MANY_PAIR_GRAMS["mixed"]
    caps = H.many_pair_gram_caps("mixed")
    plan = engine.Plan(H.capped_dims(n, caps))
    small = {i for i, c in enumerate(caps) if c <= 32}
    pr, first = plan.pairs(), plan.first_run
    assert len(pr) - first == len(small) * (len(small) + 1) // 2 >= 3 * 8 * NUM_CUS  # 6144 for the one-wave sweep
    assert all((i in small and j in small) == (t >= first) for t, (i, j) in enumerate(pr.tolist()))
    plan.close()


def test_rank_shares_hold_three_pairs_per_workgroup(built):
    from qml_cutensornet_amd import engine

    xd, yd = _dims("fused12-ranks")
    seen = set()
    for r in range(3):
        share = engine.Plan(xd, yd, 3, r)
        assert share.num_pairs >= 3 * GRID["fused12-ranks"]
        seen |= {(i, j) for i, j in share.pairs().tolist()}
        share.close()
    assert len(seen) == len(xd) * len(yd)


@pytest.mark.parametrize("name", list(H.MANY_PAIR_SETS) + list(H.MANY_PAIR_GRAMS))
def test_c_oracle_agrees_with_the_restatement_on_a_sample(built, name):
    from oracle import c_oracle
    from oracle import restatement as R

    if name in H.MANY_PAIR_GRAMS:
        xs = H.many_pair_gram_set(name)
        ys = xs
    else:
        xs, ys = H.many_pair_sets(name)
    rng = np.random.default_rng(5)
    pr = np.stack([rng.integers(0, len(xs), 50), rng.integers(0, len(ys), 50)], axis=1).astype(np.int32)
    pr[0], pr[1] = (0, 0), (len(xs) - 1, len(ys) - 1)
    v, z, _ = c_oracle.gram_pairs([m.tensors for m in xs], None if ys is xs else [m.tensors for m in ys], pr, 8)
    z_ref = np.array([R.mps_inner(xs[i].tensors, ys[j].tensors) for i, j in pr.tolist()])
    assert np.abs(z - z_ref).max() < 1e-13 and np.abs(v - np.abs(z_ref) ** 2).max() < 1e-13
