import functools
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


# ------------------------------------------------------------------ general-gauge states for the local sweeps and the sampler
# ``random_mps`` is right-orthonormal (R_k = 1) and builder output is mixed-canonical (one of L_k, R_k is the identity, the other a
# real diagonal), so neither tells a kernel that reads R transposed, conjugated or from the wrong plane from a right one.  The
# twins below hold the same states in a gauge where every L_k and R_k is dense and complex (tests/test_gauge_inputs_host.py
# asserts it), on bonds that cross the 16-row padding, the 64-wide blocks and, in ``gauge_set_300``, 300 (padded 304).
PROFILES = [  # the 20-site profiles of tests/test_gpu_entanglement.py
    [1, 2, 4, 8, 15, 16, 17, 32, 47, 48, 63, 64, 65, 128, 64, 32, 16, 8, 4, 2, 1],
    [1, 2, 4, 8, 16, 31, 48, 64, 65, 33, 17, 9, 5, 3, 2, 1, 1, 1, 1, 1, 1],
    [1, 2, 4, 8, 15, 8, 4, 2, 1, 1, 2, 3, 5, 9, 17, 16, 8, 4, 2, 2, 1],
]
PROFILE_300 = [1, 2, 4, 8, 16, 32, 64, 128, 200, 300, 150, 75, 38, 19, 10, 5, 3, 2, 1]


def scrambled(mps, rng, scale=1.0, grow=0):
    """The bounded gauge of tests/test_entanglement_host.py (G = U diag(d) V, d in [0.5, 2], cond <= 4) on every bond; with
    ``grow`` the bond becomes that much wider than before (G is chi x (chi + grow), its pseudo-inverse goes into the next site)."""
    import qml_cutensornet_amd as Q

    ts = [np.array(t, dtype=np.complex128) for t in mps.tensors]
    for k in range(1, len(ts)):
        chi = ts[k].shape[0]
        big = chi + grow
        u, _ = np.linalg.qr(rng.standard_normal((chi, chi)) + 1j * rng.standard_normal((chi, chi)))
        v, _ = np.linalg.qr(rng.standard_normal((big, big)) + 1j * rng.standard_normal((big, big)))
        d = rng.uniform(0.5, 2.0, chi)
        ts[k - 1] = np.tensordot(ts[k - 1], (u * d) @ v[:chi], axes=(2, 0))
        ts[k] = np.tensordot(v[:chi].conj().T @ ((1.0 / d)[:, None] * u.conj().T), ts[k], axes=(1, 0))
    ts[0] = ts[0] * scale
    return Q.MPS(ts)


@functools.lru_cache(maxsize=None)
def gauge_sets(seed=135):
    """(originals, twins): six ``random_mps(20, PROFILES[k % 3])`` and the same states gauge-scrambled, every second one scaled by
    3.7.  One generator, state by state (original k, twin k, original k + 1, ...): with seed 135 the twins are the mixed set of
    tests/test_gpu_compress.py."""
    import qml_cutensornet_amd as Q

    rng = np.random.default_rng(seed)
    originals, twins = [], []
    for k in range(6):
        originals.append(Q.random_mps(20, PROFILES[k % 3], rng))
        twins.append(scrambled(originals[-1], rng, scale=3.7 if k % 2 else 1.0))
    return tuple(originals), tuple(twins)


@functools.lru_cache(maxsize=None)
def gauge_set_300(seed=300):
    """(originals, twins): two ``random_mps`` on the 18-site PROFILE_300 and their scrambled twins, the second scaled by 3.7."""
    import qml_cutensornet_amd as Q

    rng = np.random.default_rng(seed)
    originals, twins = [], []
    for k in range(2):
        originals.append(Q.random_mps(18, PROFILE_300, rng))
        twins.append(scrambled(originals[-1], rng, scale=3.7 if k % 2 else 1.0))
    return tuple(originals), tuple(twins)


SHOTS = 70  # of the sampler's cases: one full tile of 64 shots and a ragged one of 6
GAUGE_SAMPLE = {"g20": (41, 7), "g300": (45, 11)}  # name: (seed of the bases, seed of the draws), chosen on the CPU: see below


def gauge_sample_case(name):
    """(states, bases (SHOTS, n), seed, index of the first twin) of a sampler case: "g20" the six twins of ``gauge_sets``, "g300"
    the two originals of ``gauge_set_300`` and then their twins.  State i is drawn with the global index i.  With these seeds no
    draw of the host mirror sits within 1e-9 of its threshold, for the case and for the originals at the twins' indices
    (tests/test_gauge_inputs_host.py asserts it; measured 5.6e-5 and 2.3e-4)."""
    from qml_cutensornet_amd import engine

    base_seed, seed = GAUGE_SAMPLE[name]
    if name == "g20":
        states, first = list(gauge_sets()[1]), 0
    else:
        originals, twins = gauge_set_300()
        states, first = list(originals) + list(twins), len(originals)
    return states, engine.random_bases(SHOTS, len(states[0]), base_seed), seed, first


def environments(tensors):
    """Plain einsum environments of one state: (L, R), lists of n + 1 matrices; L[k][ket][bra] of the sites before bond k, R[k] of
    the sites after it."""
    ts = [np.asarray(t, dtype=np.complex128) for t in tensors]
    n = len(ts)
    L, R = [None] * (n + 1), [None] * (n + 1)
    L[0] = np.ones((1, 1), dtype=np.complex128)
    R[n] = np.ones((1, 1), dtype=np.complex128)
    for k in range(n):
        L[k + 1] = np.einsum("lm,lsr,msq->rq", L[k], ts[k], ts[k].conj(), optimize=True)
    for k in range(n - 1, -1, -1):
        R[k] = np.einsum("lsr,rq,msq->lm", ts[k], R[k + 1], ts[k].conj(), optimize=True)
    return L, R


def capped_dims(n, caps):
    """The bond table [len(caps), n + 1] of capped chains (what the planner needs: no tensors)."""
    return np.array([[min(2 ** min(k, n - k), c) for k in range(n + 1)] for c in caps], dtype=np.int32)


# ------------------------------------------------------------------ canary states: a hostile neighbour, a hostile history
# (tests/test_gpu_canary.py on the GPU, tests/test_canary_host.py on the CPU).  A canary has the bond table of a clean state and NaN in
# every tensor element.  Plans, kernel choice, tiling, segmentation, queues and batch cuts depend on the bond tables alone, so a run with
# canaries walks the steps of the clean run: a result that involves no canary must be the clean run's, a result that involves one is NaN.
CANARY = complex(float("nan"), float("nan"))
CANARY_X_PERIOD, CANARY_Y_PERIOD, CANARY_Y_RESIDUE, CANARY_GRAM_PERIOD = 5, 3, 1, 5
# the canaries among the six twins of ``gauge_sets`` (local sweeps): states 1 and 4 (PROFILES[1]: bonds up to 65, one of them scaled by
# 3.7), and as a placement of its own state 3, which has the profile that reaches 128; of the two twins of ``gauge_set_300`` the first
LOCAL_CANARY_PLACEMENTS = {"1-4": (1, 4), "3": (3,)}
LOCAL_CANARIES_300 = (0,)


def canary_copy(mps):
    """A state of the same shapes with nan + 1j nan in every element."""
    import qml_cutensornet_amd as Q

    return Q.MPS([np.full(np.shape(t), CANARY, dtype=np.complex128) for t in mps.tensors])


def canary_indices(n_states, caps, period, residue=2):
    """The states of a set that become canaries: i % period == residue, never the first or the last state (the duplicates of the
    many-pairs sets stay clean), and the first inner state of the set's largest cap if none of the chosen has it."""
    caps = [int(c) for c in caps]
    assert len(caps) == n_states >= 3
    idx = [i for i in range(1, n_states - 1) if i % period == residue]
    big = max(caps)
    if not any(caps[i] == big for i in idx):
        idx.append(next(i for i in range(1, n_states - 1) if caps[i] == big))
    return sorted(idx)


def with_canaries(states, idx):
    """The list ``states`` with the entries ``idx`` replaced by their canary copies (the other entries are the same objects)."""
    idx = set(int(i) for i in idx)
    assert all(0 <= i < len(states) for i in idx)
    return [canary_copy(m) if i in idx else m for i, m in enumerate(states)]


def many_pair_canaries(name):
    """(x indices, y indices) of the canaries of MANY_PAIR_SETS[name]."""
    cx, cy = many_pair_caps(name)
    return canary_indices(len(cx), cx, CANARY_X_PERIOD), canary_indices(len(cy), cy, CANARY_Y_PERIOD, CANARY_Y_RESIDUE)


def many_pair_symmetric_canaries(name):
    """The canaries of ``many_pair_symmetric(name, xs, ys)``: those of xs, and those of ys among the states it takes."""
    cx, cy = many_pair_caps(name)
    ix, iy = many_pair_canaries(name)
    ns = len(many_pair_symmetric(name, list(range(len(cx))), list(range(len(cy)))))
    return ix + [len(cx) + j for j in iy if len(cx) + j < ns]


def many_pair_gram_canaries(name):
    """The canaries of MANY_PAIR_GRAMS[name]: period 5 and a state of the largest cap."""
    caps = many_pair_gram_caps(name)
    return canary_indices(len(caps), caps, CANARY_GRAM_PERIOD)


def canary_pair_mask(nx, ix, ny=None, iy=None):
    """bool [ny, nx]: entry (j, i) involves a canary (row j = y state, or x state of a symmetric set; column i = x state)."""
    sym = ny is None
    m = np.zeros((nx if sym else ny, nx), dtype=bool)
    m[:, list(ix)] = True
    m[list(ix if sym else iy), :] = True
    return m


# ------------------------------------------------------------------ sets that make every workgroup of the device builder take a second state
# (tests/test_gpu_builder_turns.py on the GPU, tests/test_builder_turns_host.py on the CPU).  qk_build_kernel is persistent: it launches
# min(n_states, slots) workgroups, slots = workgroups per CU x CUs, and a workgroup that has packed its state draws the next number
# from the queue -- onto the arena, the workspaces and the LDS of the state before.  A case holds slots + BUILDER_TURN_EXTRA states
# of the reference ansatz at gamma = 1 on ``R.synthetic_features(n_states, qubits, 7)``; the queue is ordered by descending proxy
# (``queue_proxy``) unless QK_BUILD_NO_ORDER is set, so which states come on a later turn is known.
BUILDER_TURN_EXTRA = 40
BUILDER_TURN_SETS = {  # name: (qubits, layers, distance, max_bond, QK_BUILD_WGS or None, workgroups per CU, threads, bond a later-turn state must reach)
    # 512 threads, the whole CU's LDS: later-turn states at bond >= 48 run the preconditioned block factorisation, the Gram-Schmidt
    # centre moves and the theta product on the matrix cores
    "wide": (12, 4, 3, 64, "1", 1, 512, 48),
    # two workgroups of 256 threads: the block path at >= 48 columns (bond >= 24)
    "two": (10, 3, 3, 64, "2", 2, 256, 24),
    # four workgroups, the default at max_bond <= 32: a 48-column theta no longer fits the 38 KiB and is factorised from L2
    "four": (10, 3, 3, 32, None, 4, 256, 24),
}
# the partial build: the circuits of "two" in the 512-thread shape with a cap that some states outgrow and some do not, so that on
# one workgroup a dropped state is followed by an ordinary one and the other way round.  (circuits of, QK_BUILD_WGS, workgroups per
# CU, threads, max_bond, least number of dropped and of ordinary states among the later-turn positions and of dropped ones among
# the first slots.)  A state is dropped when a bond outgrows the cap at ANY gate (``outgrows``), not only when a final bond does: by
# final bonds 210 of the 256 heaviest states and 14 of the 40 lightest lie above 28, by the largest bond on the way 225 and 21.
BUILDER_TURN_PARTIAL = ("two", "1", 1, 512, 28, 16)
# a build that truncates, beyond the slots: the circuits of "two" in the two-workgroup shape cut at bond 8 (``truncate=True``).  In the
# default order nearly every first-turn state loses more than 1e-6 of fidelity and about half of the later-turn states lose less, so a
# fidelity carried from one state of a workgroup into the next is wrong by far more than any tolerance, whether or not the builder
# repeats its bits.  (circuits of, max_bond, least share of first-turn states and least number of later-turn states below 1 - 1e-6)
BUILDER_TURN_TRUNCATE = ("two", 8, 0.75, 16)
BUILDER_TURN_SEED = 7


def builder_turn_circuits(name, slots, extra=BUILDER_TURN_EXTRA):
    """The slots + extra bound circuits of BUILDER_TURN_SETS[name]."""
    import qml_cutensornet_amd as Q
    from oracle import restatement as R

    n, reps, d = BUILDER_TURN_SETS[name][:3]
    ans = Q.KernelStateAnsatz(n, reps, 1.0, Q.entanglement_graph(n, d))
    return [ans.circuit_for_data(x) for x in R.synthetic_features(slots + extra, n, BUILDER_TURN_SEED)]


def queue_proxy(circuit):
    """The cost proxy the device builder orders its queue by: sin^2(pi alpha) summed over the XXPhase, YYPhase and ZZPhase gates."""
    op, alpha = np.asarray(circuit.op), np.asarray(circuit.alpha, dtype=np.float64)
    return float((np.sin(np.pi * alpha[(op == 2) | (op == 6) | (op == 7)]) ** 2).sum())


def queue_order(circuits, ordered=True):
    """The state at every queue position: by descending proxy, ties in input order (``ordered``), or the input order
    (QK_BUILD_NO_ORDER)."""
    if not ordered:
        return np.arange(len(circuits))
    return np.argsort(-np.array([queue_proxy(c) for c in circuits]), kind="stable")


def later_turn_states(circuits, slots, ordered=True):
    """The states at queue positions >= slots: whoever takes them has built a state before."""
    return queue_order(circuits, ordered)[slots:]


def ascending_by_proxy(circuits):
    """The permutation that sorts the circuits by ascending proxy: under QK_BUILD_NO_ORDER the heavy states then come last, onto
    arenas that held light ones."""
    return np.argsort(np.array([queue_proxy(c) for c in circuits]), kind="stable")


def host_states(circuits, max_bond=None):
    """The host builder's states of the circuits (``simulate_many`` on up to 16 cores)."""
    from qml_cutensornet_amd import mps

    return mps.simulate_many(circuits, 1 - 1e-16, workers=min(16, os.cpu_count() or 1), max_bond=max_bond)[0]


def outgrows(circuits, cap, host=None):
    """bool per circuit: does a bond of the host builder's state exceed ``cap`` after any gate -- what makes the device builder drop
    the state in a partial build.  ``host``: the finished host states, if at hand (a final bond above the cap settles it; the others
    are walked with a checkpoint behind every two-qubit gate)."""
    import qml_cutensornet_amd as Q

    host = host_states(circuits) if host is None else host
    out = np.array([m.max_bond() > cap for m in host])
    for k, c in enumerate(circuits):
        if not out[k]:
            cps = sorted(set((np.flatnonzero(np.isin(np.asarray(c.op), (2, 3, 6, 7, 9, 11))) + 1).tolist()) | {c.n_gates})
            out[k] = max(m.max_bond() for m in Q.simulate(c, 1 - 1e-16, checkpoints=cps)) > cap
    return out
