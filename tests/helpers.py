import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(name):
    return np.load(os.path.join(GOLDEN, name))


def golden_mps_sets():
    g = golden("mps_pairs_9q.npz")
    n = int(g["n"])
    sets = {tag: [g[f"{tag}_{k}"] for k in range(n)] for tag in ("x0", "x1", "y0", "y1")}
    return [sets["x0"], sets["x1"]], [sets["y0"], sets["y1"]], g["z"]


# ------------------------------------------------------------------ sets whose sweeps make every workgroup take many pairs
# (tests/test_gpu_many_pairs.py on the GPU, tests/test_many_pairs_host.py on the CPU).  Random chains with capped profiles
# min(2^min(k, n - k), cap); state i of a set has the cap caps[i % len(caps)], so neighbours in a work queue differ in tiles, in where X
# lives (LDS in place, ping-pong, the global buffer), in k-tails (1..3 k-steps in the last block of rows) and in the parity of the column
# blocks.  The LAST state of every set is its FIRST one again (the duplicate checks).
def capped_mps(n, cap, rng):
    import qml_cutensornet_amd as Q

    return Q.random_mps(n, [min(2 ** min(k, n - k), cap) for k in range(n + 1)], rng)


MANY_PAIR_SETS = {  # name: (sites, x caps, y caps, x states, y states, seed)
    # the 12-wave shapes (dual, one-tile): 112 x 80 and more = global X in strips, 3 = a single block, 17 / 33 / 22 / 70 / 100 / 9 = k-tails
    "fused12": (14, (112, 17, 64, 100, 33, 3, 90, 48, 128, 22, 70, 40), (16, 48, 70, 128, 9, 100, 33, 64), 36, 24, 101),
    "fused12-ranks": (14, (112, 17, 64, 100, 33, 3, 90, 48, 128, 22, 70, 40), (16, 48, 70, 128, 9, 100, 33, 64), 54, 48, 102),
    # the two-workgroup shape: every site fits its 4608-element buffer (48 x 48 twice: exactly), one to three blocks a side
    "fused8": (12, (48, 17, 36, 3, 40, 22, 33, 9), (33, 48, 16, 40, 5, 36, 24, 44), 40, 40, 103),
    # the one-wave sweep with 2 x 2 register tiles: one and two blocks a side, long chains
    "wave2": (24, (32, 17, 24, 3, 29, 20, 9, 31), (18, 32, 5, 27, 16, 30, 22, 11), 80, 80, 104),
    # the one-wave register sweep: a single block
    "wave": (12, (16, 3, 9, 12, 5, 14, 2, 7), (7, 16, 4, 11, 13, 3, 15, 8), 112, 112, 105),
}
# symmetric sets: state i has the cap caps[i]; the last state is the first one again
MANY_PAIR_GRAMS = {  # name: (sites, caps, seed)
    # two launches (QK_FUSED_SPLIT=2): the pairs with a large state for the 12-wave shape, the small-small ones for two workgroups per CU
    "split": (16, [(40, 48, 56, 60, 33, 20, 52, 36)[i % 8] for i in range(60)] + [(150, 120, 100, 64, 90, 140, 80, 112)[i % 8] for i in range(13)], 106),
    # a mixed set: the pairs of two states with every bond <= 32 are the second run, for the one-wave sweep
    "mixed": (16, [(30, 24, 17, 32, 9, 28, 31, 12, 20, 26, 16, 29)[i % 12] for i in range(112)] + [90, 140, 60], 107),
}


def many_pair_caps(name):
    """The caps of the x and of the y states of a set, duplicates included."""
    _, xc, yc, nx, ny, _ = MANY_PAIR_SETS[name]
    cx, cy = [xc[i % len(xc)] for i in range(nx)], [yc[j % len(yc)] for j in range(ny)]
    cx[-1], cy[-1] = cx[0], cy[0]
    return cx, cy


def many_pair_sets(name):
    """(xs, ys) of MANY_PAIR_SETS[name]: lists of MPS; xs[-1] is xs[0] and ys[-1] is ys[0]."""
    n, _, _, _, _, seed = MANY_PAIR_SETS[name]
    rng = np.random.default_rng(seed)
    cx, cy = many_pair_caps(name)
    xs = [capped_mps(n, c, rng) for c in cx[:-1]]
    ys = [capped_mps(n, c, rng) for c in cy[:-1]]
    return xs + [xs[0]], ys + [ys[0]]


def many_pair_gram_caps(name):
    caps = list(MANY_PAIR_GRAMS[name][1])
    caps[-1] = caps[0]
    return caps


def many_pair_gram_set(name):
    """The states of MANY_PAIR_GRAMS[name]; the last one is the first one."""
    n, _, seed = MANY_PAIR_GRAMS[name]
    rng = np.random.default_rng(seed)
    xs = [capped_mps(n, c, rng) for c in many_pair_gram_caps(name)[:-1]]
    return xs + [xs[0]]


def many_pair_symmetric(name, xs, ys):
    """The symmetric set of a rectangular case: xs and as many of ys as make its Gram as long as the rectangle (at least)."""
    nx, ny = len(xs), len(ys)
    k = next(k for k in range(ny + 1) if (nx + k) * (nx + k + 1) // 2 >= nx * ny or k == ny)
    return xs + ys[:k]


def capped_dims(n, caps):
    """The bond table [len(caps), n + 1] of capped chains (what the planner needs: no tensors)."""
    return np.array([[min(2 ** min(k, n - k), c) for k in range(n + 1)] for c in caps], dtype=np.int32)
