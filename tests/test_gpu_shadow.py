"""GPU tier: the classical-shadow kernel's shot-pair histograms (qk_shadow_hist_host, Context.shadow_hist_host / shadow_hists,
build_shadow_kernel_matrix).  Everything is integer arithmetic, so every case is ``np.array_equal`` against the numpy mirror
``engine.shadow_hist``: the shapes where a lane, wave, group, staging or layout boundary sits (one histogram per wave up to 2^14 shot
pairs per pair of states, per-lane counters beyond), pair lists, symmetric and rectangular calls, shared and per-state bases, known
answers where one bin takes every increment, the equal-shot histograms, shots of device-resident states end to end, the rejections and
the distributed route, one rank against two bit for bit.  Definitions: tests/test_shadow_host.py, include/qkgram.h."""
import os
import sys

import numpy as np
import pytest

import qml_cutensornet_amd as Q
from oracle import restatement as R
from qml_cutensornet_amd import engine
from test_shadow_host import END_TO_END, end_to_end_case, random_shots, upper_pairs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUBITS = (1, 5, 31, 32, 33, 64, 65, 128)
DIST = {"n": 8, "layers": 2, "nx": 7, "ny": 4, "shots": 32, "seed": 5}


def both(gpu_ctx, bx, cx, by, cy, pairs):
    """device and mirror histograms with their equal-shot parts where the shots allow them"""
    eq = by is None or by.shape[1] == bx.shape[1]
    got = gpu_ctx.shadow_hist_host(bx, cx, by, cy, pairs, equal=eq)
    want = engine.shadow_hist(bx, cx, by, cy, pairs, equal=eq)
    if not eq:
        got, want = (got, None), (want, None)
    assert got[0].dtype == np.int64 and np.all(got[0].sum(axis=1) == bx.shape[1] * (bx if by is None else by).shape[1])
    return got, want


def same(got, want):
    return all((g is None and w is None) or np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 257])
def test_single_pair_shapes(gpu_ctx, T):
    # up to 65 shots a pair of states has at most 2^14 shot pairs (one histogram per wave); 257 takes the per-lane counters
    rng = np.random.default_rng(100 + T)
    for n in QUBITS:
        bits, bases = random_shots(rng, 2, T, n)
        got, want = both(gpu_ctx, bits, bases, None, None, [(0, 1)])
        assert same(got, want), n


def test_layout_boundary_and_unequal_shots(gpu_ctx):
    rng = np.random.default_rng(1)
    # 128 x 128 = 2^14 shot pairs is the last shared case, 128 x 129 the first private one; T_x != T_y both ways round
    for n, tx, ty in ((7, 128, 128), (7, 128, 129), (60, 129, 128), (33, 3, 300), (65, 300, 3), (128, 70, 259), (100, 200, 130), (5, 1, 64)):
        bx, cx = random_shots(rng, 2, tx, n)
        by, cy = random_shots(rng, 3, ty, n, per_state=True)
        got, want = both(gpu_ctx, bx, cx, by, cy, [(1, 2), (0, 0)])
        assert same(got, want), (n, tx, ty)


def test_pair_lists(gpu_ctx):
    rng = np.random.default_rng(2)
    for T in (10, 140):  # both layouts
        bits, bases = random_shots(rng, 6, T, 7)
        one = gpu_ctx.shadow_hist_host(bits, bases, pairs=[(4, 2)])
        assert one.shape == (1, 15) and np.array_equal(one, engine.shadow_hist(bits, bases, None, None, [(4, 2)]))
        # unordered, with duplicates and self pairs
        pairs = [(5, 0), (1, 1), (0, 5), (5, 0), (3, 3), (2, 4), (1, 1), (0, 0)]
        got, want = both(gpu_ctx, bits, bases, None, None, pairs)
        assert same(got, want)
        assert np.array_equal(got[0][0], got[0][3]) and np.array_equal(got[0][0], got[0][2])  # d is symmetric in its two shots
        assert got[1][1][14] == T and got[1][1].sum() == T  # a self pair's t = t' terms: a shot with itself, d = n
    # more tasks than one launch holds
    many, bases = random_shots(rng, 60, 2, 6)
    idx = rng.integers(0, 60, size=(3000, 2))
    got, want = both(gpu_ctx, many, bases, None, None, idx)
    assert same(got, want)


def test_long_tables_and_known_answers(gpu_ctx):
    rng = np.random.default_rng(3)
    T = 4100  # a y table longer than one staging pass, 65 x blocks, several tasks for the one pair
    for n in (5, 40):
        bits, bases = random_shots(rng, 2, T, n)
        got, want = both(gpu_ctx, bits, bases, None, None, [(0, 1)])
        assert same(got, want), n
    # one bin takes every increment: 4100^2 = 16 810 000 of them
    n = 70
    row, codes = rng.integers(0, 2, size=n, dtype=np.uint8), rng.integers(1, 4, size=n, dtype=np.uint8)
    bits, bases = np.tile(row, (1, T, 1)), np.tile(codes, (T, 1))

    def only(bin_):
        want = np.zeros((1, 2 * n + 1), dtype=np.int64)
        want[0, bin_] = T * T
        return want

    assert np.array_equal(gpu_ctx.shadow_hist_host(bits, bases, bits, bases, [(0, 0)]), only(2 * n))  # identical constant tables
    assert np.array_equal(gpu_ctx.shadow_hist_host(bits, bases, 1 - bits, bases, [(0, 0)]), only(0))  # complemented outcomes
    z, x = np.full((T, n), 3, dtype=np.uint8), np.full((T, n), 1, dtype=np.uint8)
    assert np.array_equal(gpu_ctx.shadow_hist_host(bits, z, bits, x, [(0, 0)]), only(n))  # all Z against all X
    # the same three where a wave shares one histogram
    small, sb = bits[:, :50], bases[:50]
    want = np.zeros((1, 2 * n + 1), dtype=np.int64)
    want[0, 2 * n] = 2500
    assert np.array_equal(gpu_ctx.shadow_hist_host(small, sb, small, sb, [(0, 0)]), want)
    assert np.array_equal(gpu_ctx.shadow_hist_host(small, sb, 1 - small, sb, [(0, 0)]), want[:, ::-1])
    assert np.array_equal(gpu_ctx.shadow_hist_host(small, z[:50], small, x[:50], [(0, 0)]), np.roll(want, -n, axis=1))


def test_symmetric_and_rectangular_calls(gpu_ctx):
    rng = np.random.default_rng(4)
    n, T = 9, 20
    bx, cx = random_shots(rng, 5, T, n)
    by, cy = random_shots(rng, 3, T, n)
    pairs = [(i, j) for j in range(3) for i in range(5)]
    got, want = both(gpu_ctx, bx, cx, by, cy, pairs)
    assert same(got, want)
    # equal on and off give the same histograms
    assert np.array_equal(gpu_ctx.shadow_hist_host(bx, cx, by, cy, pairs), got[0])
    # a rectangular call on the same table gives what the symmetric call gives
    rect = gpu_ctx.shadow_hist_host(bx, cx, bx, cx, [(2, 2), (1, 2)], equal=True)
    sym = gpu_ctx.shadow_hist_host(bx, cx, pairs=[(2, 2), (1, 2)], equal=True)
    assert same(rect, sym) and same(sym, engine.shadow_hist(bx, cx, None, None, [(2, 2), (1, 2)], equal=True))
    # shadow_hists: (ny, nx, 2 n + 1), mirrored when symmetric
    H, E = gpu_ctx.shadow_hists(bx, cx, equal=True)
    assert H.shape == E.shape == (5, 5, 2 * n + 1) and np.array_equal(H, H.transpose(1, 0, 2)) and np.array_equal(E, E.transpose(1, 0, 2))
    up = upper_pairs(5)
    wh, we = engine.shadow_hist(bx, cx, None, None, up, equal=True)
    assert np.array_equal(H[up[:, 1], up[:, 0]], wh) and np.array_equal(E[up[:, 1], up[:, 0]], we)
    H2 = gpu_ctx.shadow_hists(bx, cx, by, cy)
    assert H2.shape == (3, 5, 2 * n + 1) and np.array_equal(H2, want[0].reshape(3, 5, -1))
    H2, E2 = gpu_ctx.shadow_hists(bx, cx, by, cy, equal=True)
    assert np.array_equal(H2, want[0].reshape(3, 5, -1)) and np.array_equal(E2, want[1].reshape(3, 5, -1))
    K = engine.shadow_kernel(H, n, equal=E)
    assert K.shape == (5, 5) and np.array_equal(K, K.T)


def test_shared_against_per_state_bases(gpu_ctx):
    rng = np.random.default_rng(5)
    for n, T in ((33, 12), (60, 150)):
        bx, cx = random_shots(rng, 3, T, n)
        by, cy = random_shots(rng, 2, T, n)
        pairs = [(0, 1), (2, 0), (1, 1)]
        shared = gpu_ctx.shadow_hist_host(bx, cx, by, cy, pairs, equal=True)
        per = gpu_ctx.shadow_hist_host(bx, np.broadcast_to(cx, bx.shape), by, np.broadcast_to(cy, by.shape), pairs, equal=True)
        mixed = gpu_ctx.shadow_hist_host(bx, cx, by, np.broadcast_to(cy, by.shape), pairs, equal=True)
        assert same(shared, per) and same(shared, mixed) and same(shared, engine.shadow_hist(bx, cx, by, cy, pairs, equal=True))


def test_batch_cap_and_trim(gpu_ctx, monkeypatch):
    rng = np.random.default_rng(6)
    for n, T in ((40, 9), (40, 130)):
        bits, bases = random_shots(rng, 4, T, n)
        pairs = upper_pairs(4)
        free = gpu_ctx.shadow_hist_host(bits, bases, pairs=pairs, equal=True)
        monkeypatch.setenv("QK_SHADOW_BATCH", "1")
        one = gpu_ctx.shadow_hist_host(bits, bases, pairs=pairs, equal=True)
        monkeypatch.setenv("QK_SHADOW_BATCH", "3")
        three = gpu_ctx.shadow_hist_host(bits, bases, pairs=pairs, equal=True)
        monkeypatch.setenv("QK_SHADOW_BATCH", "0")
        with pytest.raises(engine.QkError, match="QK_SHADOW_BATCH"):
            gpu_ctx.shadow_hist_host(bits, bases, pairs=pairs)
        monkeypatch.delenv("QK_SHADOW_BATCH")
        assert same(free, one) and same(free, three) and same(free, engine.shadow_hist(bits, bases, None, None, pairs, equal=True))
        gpu_ctx.trim()  # the pair batch's scratch goes back; the next call takes it again
        assert same(gpu_ctx.shadow_hist_host(bits, bases, pairs=pairs, equal=True), free)


def test_end_to_end_on_device_shots(gpu_ctx):
    c = END_TO_END
    states, B, host_bits = end_to_end_case()
    pairs = upper_pairs(len(states))
    with gpu_ctx.upload(states) as xs:
        bits = gpu_ctx.sample(xs, c["shots"], bases=B, seed=c["shot_seed"])
    assert np.array_equal(bits, host_bits)
    H, E = gpu_ctx.shadow_hists(bits, B, equal=True)
    wh, we = engine.shadow_hist(host_bits, B, None, None, pairs, equal=True)
    assert np.array_equal(H[pairs[:, 1], pairs[:, 0]], wh) and np.array_equal(E[pairs[:, 1], pairs[:, 0]], we)
    assert np.array_equal(engine.shadow_kernel(H, c["n"])[pairs[:, 1], pairs[:, 0]], engine.shadow_kernel(wh, c["n"]))


def test_rejections(gpu_ctx):
    rng = np.random.default_rng(12)
    bx, cx = random_shots(rng, 2, 3, 5)
    by, cy = random_shots(rng, 2, 4, 5)
    for change, match in (
        (dict(pairs=[(0, 2)]), r"pairs\[0\]"),
        (dict(pairs=[(0, 1), (-1, 0)]), r"pairs\[1\]"),
        (dict(pairs=[]), "n_pairs"),
        (dict(bits_x=bx + 2), "bits_x holds a bit other than 0 or 1"),
        (dict(bases_x=cx * 0), "bases_x holds a basis code outside"),
        (dict(bases_x=cx + 3), "bases_x holds a basis code outside"),
        (dict(bits_y=by * 3, bases_y=cy), "bits_y holds a bit other than 0 or 1"),
        (dict(bits_y=by, bases_y=cy + 1), "bases_y holds a basis code outside"),
        (dict(bases_y=cx), "bases_y is given"),
        (dict(bits_y=by, bases_y=cy, equal=True), "equal needs shots_x == shots_y"),
    ):
        kw = {**dict(bits_x=bx, bases_x=cx, bits_y=None, bases_y=None, pairs=[(0, 1)]), **change}
        with pytest.raises(engine.QkError, match=match):
            gpu_ctx.shadow_hist_host(**kw)
    wide, wb = random_shots(rng, 1, 2, 129)
    with pytest.raises(engine.QkError, match="n_sites must be <= 128"):
        gpu_ctx.shadow_hist_host(wide, wb, pairs=[(0, 0)])
    with pytest.raises(ValueError, match="bases_y"):
        gpu_ctx.shadow_hist_host(bx, cx, by, None, [(0, 1)])
    # the raw entry point: null arguments, counts below 1, flags
    L, h = engine.lib(), gpu_ctx.handle
    bits, bases, ybits, ybases = (np.ascontiguousarray(a) for a in (bx, cx, by, cy))
    pairs, hist = np.zeros((1, 2), dtype=np.int32), np.zeros((1, 11), dtype=np.int64)
    good = [h, 5, 2, 3, bits.ctypes.data, bases.ctypes.data, 0, 2, 3, None, None, 0, 1, pairs.ctypes.data, hist.ctypes.data, None]
    assert L.qk_shadow_hist_host(*good) == 0 and hist.sum() == 9
    for at, value, match in ((0, None, "ctx"), (4, None, "bits_x"), (5, None, "bases_x"), (13, None, "pairs"), (14, None, "hist"), (1, 0, "n_sites"), (1, 129, "n_sites"),
                             (2, 0, "nx"), (3, 0, "shots_x"), (7, 0, "ny"), (8, 0, "shots_y"), (12, 0, "n_pairs"), (7, 3, "ny 3 != nx 2"), (8, 4, "shots_y 4 != shots_x 3"),
                             (10, ybases.ctypes.data, "bases_y is given"), (6, 2, "bases_x_per_state"), (11, -1, "bases_y_per_state")):
        args = list(good)
        args[at] = value
        assert L.qk_shadow_hist_host(*args) != 0
        assert match in L.qk_last_error().decode(), (at, L.qk_last_error())
    rect = list(good)
    rect[8], rect[9] = 4, ybits.ctypes.data
    assert L.qk_shadow_hist_host(*rect) != 0 and "bases_y is null" in L.qk_last_error().decode()
    rect[10] = ybases.ctypes.data
    assert L.qk_shadow_hist_host(*rect) == 0 and hist.sum() == 12
    rect[15] = hist.ctypes.data
    assert L.qk_shadow_hist_host(*rect) != 0 and "equal" in L.qk_last_error().decode()


def _dist_inputs(Q_, R_):
    n = DIST["n"]
    ans = Q_.KernelStateAnsatz(n, DIST["layers"], 1.0, Q_.entanglement_graph(n, 2))
    return ans, R_.synthetic_features(DIST["nx"], n, 13), R_.synthetic_features(DIST["ny"], n, 14)


def _dist_runs(build, comm, ans, X, Y):
    kw = dict(shots=DIST["shots"], shot_seed=DIST["seed"], truncation_error=1e-16, return_hist=True)
    return {"train": build(comm, ans, X, **kw), "test": build(comm, ans, X, Y, shadow_gamma=0.5, shadow_tau=2.0, skip_equal_shots=False, **kw)}


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["QK_BUILDER"] = "host"
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import qml_cutensornet_amd as Q_
        from oracle import restatement as R_
        from qml_cutensornet_amd.dist import TorchComm
        from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_shadow_kernel_matrix

        q.put((rank, _dist_runs(build_shadow_kernel_matrix, TorchComm(), *_dist_inputs(Q_, R_))))
    finally:
        dist.destroy_process_group()


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    return np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.timeout(300)
def test_two_ranks_match_one_rank_bitwise(built, monkeypatch):
    import torch.multiprocessing as mp

    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_shadow_kernel_matrix

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + ((os.getpid() + 1733) % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert res[1]["train"] is None and res[1]["test"] is None
    monkeypatch.setenv("QK_BUILDER", "host")
    one = _dist_runs(build_shadow_kernel_matrix, SingleComm(), *_dist_inputs(Q, R))
    for which in ("train", "test"):
        assert _same(res[0][which], one[which]), which


def test_build_shadow_kernel_matrix_against_its_pieces(built, gpu_ctx, monkeypatch):
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_shadow_kernel_matrix

    monkeypatch.setenv("QK_BUILDER", "host")
    ans, X, Y = _dist_inputs(Q, R)
    n, T, seed = DIST["n"], DIST["shots"], DIST["seed"]
    out = _dist_runs(build_shadow_kernel_matrix, SingleComm(), ans, X, Y)
    # against the pieces: the states of Y are sampled with indices after those of X, every state in the same bases
    xs = [Q.simulate(ans.circuit_for_data(x), 1 - 1e-16) for x in X]
    ys = [Q.simulate(ans.circuit_for_data(y), 1 - 1e-16) for y in Y]
    B = engine.random_bases(T, n, seed)
    bx = np.stack([m.sample(T, bases=B, seed=seed, state_index=s) for s, m in enumerate(xs)])
    by = np.stack([m.sample(T, bases=B, seed=seed, state_index=len(xs) + s) for s, m in enumerate(ys)])
    (K, parts), (Kt, parts_t) = out["train"], out["test"]
    H, E = gpu_ctx.shadow_hists(bx, B, equal=True)
    assert np.array_equal(parts["hist"], H) and np.array_equal(parts["equal"], E)
    assert np.array_equal(K, engine.shadow_kernel(H, n, 1.0, 1.0, equal=E)) and np.array_equal(K, K.T) and K.shape == (len(X), len(X))
    H, E = gpu_ctx.shadow_hists(bx, B, by, B, equal=True)
    assert np.array_equal(parts_t["hist"], H) and np.array_equal(parts_t["equal"], E)
    assert np.array_equal(Kt, engine.shadow_kernel(H, n, 0.5, 2.0)) and Kt.shape == (len(Y), len(X))
    # without return_hist: K alone
    K2 = build_shadow_kernel_matrix(SingleComm(), ans, X, shots=T, shot_seed=seed, truncation_error=1e-16)
    assert isinstance(K2, np.ndarray) and np.array_equal(K2, K)
    for kwargs, match in ((dict(shots=1), "shots"), (dict(shots=None), "shots"), (dict(shots=True), "shots"), (dict(shots=8.0), "shots"), (dict(shots=8, shadow_gamma=np.inf), "shadow_gamma")):
        with pytest.raises(ValueError, match=match):
            build_shadow_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, **kwargs)
    wide = Q.KernelStateAnsatz(129, 1, 1.0, Q.entanglement_graph(129, 1))
    with pytest.raises(ValueError, match="128"):
        build_shadow_kernel_matrix(SingleComm(), wide, np.zeros((2, 129)), shots=8, truncation_error=1e-16)
