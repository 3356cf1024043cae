"""GPU tier: block overlaps at finite shots (qk_shot_block_sums_host, Context.shot_block_sums_host / shot_block_overlaps,
build_block_kernel_matrices(shots=...)).  Everything is integer arithmetic, so every case is ``np.array_equal`` against the numpy
mirror ``engine.shot_block_sums``: the shapes where a lane, wave, workgroup, word or staging boundary sits, pair lists, symmetric and
rectangular calls, known answers (one beyond 2^32), the per-setting sums, shots of device-resident states end to end, the rejections
and the distributed route, one rank against two bit for bit.  Definitions: tests/test_shot_block_host.py, include/qkgram.h."""
import os
import sys

import numpy as np
import pytest

import qml_cutensornet_amd as Q
from oracle import restatement as R
from qml_cutensornet_amd import engine
from test_shot_block_host import END_TO_END, SIDES, exact_block_overlaps, random_tables, shot_case, upper_pairs, within_four_stderr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = {1: [1], 5: [1, 2, 5], 32: [1, 31, 32], 33: [1, 31, 32], 40: [1, 16, 31, 32]}
DIST = {"n": 8, "layers": 2, "nx": 7, "ny": 4, "shots": (8, 16), "seed": 5, "widths": (1, 3, 8)}


def both(gpu_ctx, bx, by, U, pairs, widths, side):
    """device and mirror sums with their per-setting parts, after checking the device's parts against its sums"""
    got, got_S = gpu_ctx.shot_block_sums_host(bx, by, U, pairs, widths, side, per_setting=True)
    want, want_S = engine.shot_block_sums(bx, by, U, pairs, widths, side, per_setting=True)
    assert got.dtype == np.int64 and got_S.dtype == np.int64 and np.array_equal(got_S.sum(axis=2), got)
    return got, got_S, want, want_S


@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 257])
def test_single_pair_shapes(gpu_ctx, M):
    rng = np.random.default_rng(100 + M)
    for U in (1, 3):
        for n, widths in WIDTHS.items():
            bits = random_tables(rng, 2, U, M, n)
            for side in SIDES:
                got, got_S, want, want_S = both(gpu_ctx, bits, None, U, [(0, 1)], widths, side)
                assert np.array_equal(got, want) and np.array_equal(got_S, want_S), (U, n, side)


def test_every_width_of_a_word(gpu_ctx):
    # 32 widths: four launches of eight; 7 widths: launches of 4, 2 and 1
    bits = random_tables(np.random.default_rng(1), 3, 2, 9, 32)
    for widths in (list(range(1, 33)), [1, 2, 3, 5, 8, 13, 21]):
        got, got_S, want, want_S = both(gpu_ctx, bits, None, 2, [(0, 1), (2, 2), (1, 0)], widths, "right")
        assert np.array_equal(got, want) and np.array_equal(got_S, want_S)


def test_pair_lists(gpu_ctx):
    rng = np.random.default_rng(2)
    bits = random_tables(rng, 6, 3, 10, 7)
    one = gpu_ctx.shot_block_sums_host(bits, None, 3, [(4, 2)], [1, 4, 7])
    assert one.shape == (3, 1) and np.array_equal(one, engine.shot_block_sums(bits, None, 3, [(4, 2)], [1, 4, 7]))
    # unordered, with duplicates and self pairs
    pairs = [(5, 0), (1, 1), (0, 5), (5, 0), (3, 3), (2, 4), (1, 1), (0, 0)]
    got, got_S, want, want_S = both(gpu_ctx, bits, None, 3, pairs, [1, 4, 7], "left")
    assert np.array_equal(got, want) and np.array_equal(got_S, want_S)
    assert np.array_equal(got[:, 0], got[:, 3]) and np.array_equal(got[:, 0], got[:, 2])  # the estimator is symmetric in its two tables
    # more tasks than one launch holds
    many = random_tables(rng, 60, 1, 2, 6)
    idx = rng.integers(0, 60, size=(3000, 2))
    got, got_S, want, want_S = both(gpu_ctx, many, None, 1, idx, [2, 6], "left")
    assert np.array_equal(got, want) and np.array_equal(got_S, want_S)


def test_many_settings_per_task_and_long_rows(gpu_ctx):
    rng = np.random.default_rng(3)
    # enough pairs that a task takes a chunk of many settings, the last chunk ragged
    bits = random_tables(rng, 60, 70, 3, 5)
    pairs = upper_pairs(60)
    got, got_S, want, want_S = both(gpu_ctx, bits, None, 70, pairs, [1, 5], "right")
    assert np.array_equal(got, want) and np.array_equal(got_S, want_S)
    # a row of y words longer than a workgroup stages at once
    long_bits = random_tables(rng, 2, 1, 4100, 5)
    got, got_S, want, want_S = both(gpu_ctx, long_bits, None, 1, [(0, 1)], [2, 5], "left")
    assert np.array_equal(got, want) and np.array_equal(got_S, want_S)
    # so many terms per lane that the fp64 partial sums are moved into the int64 totals on the way: y is one string throughout, so the
    # sum is M times the sum over the x shots
    M, n = 17000, 32
    x = random_tables(rng, 1, 1, M, n)
    y = np.repeat(random_tables(rng, 1, 1, 1, n), M, axis=1)
    words_x, word_y = engine.pack_block_words(x[0]), engine.pack_block_words(y[0, :1])
    want = []
    for w in (7, 32):
        D = np.array([bin(int(v) & ((1 << w) - 1)).count("1") for v in words_x ^ word_y])
        want.append(M * int(np.sum((1 - 2 * (D & 1)) * (np.int64(1) << (w - D)))))
    got = gpu_ctx.shot_block_sums_host(x, y, 1, [(0, 0)], [7, 32])
    assert [int(v) for v in got[:, 0]] == want


def test_symmetric_and_rectangular_calls(gpu_ctx):
    rng = np.random.default_rng(4)
    U, M, n = 4, 6, 9
    bx, by = random_tables(rng, 5, U, M, n), random_tables(rng, 3, U, M, n)
    pairs = [(i, j) for j in range(3) for i in range(5)]
    got, got_S, want, want_S = both(gpu_ctx, bx, by, U, pairs, [1, 9], "left")
    assert np.array_equal(got, want) and np.array_equal(got_S, want_S)
    # in a rectangular call equal indices are not a self pair, even on the same table
    rect = gpu_ctx.shot_block_sums_host(bx, bx, U, [(2, 2), (1, 2)], [1, 9])
    sym = gpu_ctx.shot_block_sums_host(bx, None, U, [(2, 2), (1, 2)], [1, 9])
    assert np.array_equal(rect, engine.shot_block_sums(bx, bx, U, [(2, 2), (1, 2)], [1, 9]))
    assert np.array_equal(sym, engine.shot_block_sums(bx, None, U, [(2, 2), (1, 2)], [1, 9]))
    assert [int(v) for v in rect[:, 0] - sym[:, 0]] == [U * M * 2, U * M * 2 ** 9] and np.array_equal(rect[:, 1], sym[:, 1])
    # shot_block_overlaps: shapes of block_overlaps, mirrored, the diagonal the purity estimate
    (O, Sx, Sy), (E, Ex, Ey) = gpu_ctx.shot_block_overlaps(bx, None, U, [1, 9], "left", stderr=True)
    assert O.shape == E.shape == (2, 5, 5) and Sx.shape == (2, 5) and Sy is Sx and Ey is Ex
    assert np.array_equal(O, O.transpose(0, 2, 1)) and np.array_equal(O[:, np.arange(5), np.arange(5)], Sx)
    up = upper_pairs(5)
    s, S = engine.shot_block_sums(bx, None, U, up, [1, 9], "left", per_setting=True)
    o, e = engine.shot_block_estimate(s, S, U, M, up[:, 0] == up[:, 1])
    assert np.array_equal(O[:, up[:, 1], up[:, 0]], o) and np.array_equal(E[:, up[:, 1], up[:, 0]], e)
    O2, Sx2, Sy2 = gpu_ctx.shot_block_overlaps(bx, by, U, [1, 9], "left")
    assert O2.shape == (2, 3, 5) and Sx2.shape == (2, 5) and Sy2.shape == (2, 3) and np.array_equal(Sx2, Sx)
    assert np.array_equal(O2, engine.shot_block_estimate(want, None, U, M, False)[0].reshape(2, 3, 5))
    assert np.array_equal(Sy2, gpu_ctx.shot_block_overlaps(by, None, U, [1, 9], "left")[1])


@pytest.mark.parametrize("side", SIDES)
def test_known_answers(gpu_ctx, side):
    rng = np.random.default_rng(7)
    U, M, n = 3, 5, 9
    widths = [1, 2, 8, 9]
    same = np.repeat(random_tables(rng, 1, U, 1, n), M, axis=1)
    two = np.concatenate([same, same])
    sums = gpu_ctx.shot_block_sums_host(two, None, U, [(0, 1), (1, 1)], widths, side)
    assert [int(v) for v in sums[:, 0]] == [U * M * M * 2 ** w for w in widths]
    assert [int(v) for v in sums[:, 1]] == [U * M * (M - 1) * 2 ** w for w in widths]
    sums = gpu_ctx.shot_block_sums_host(same, 1 - same, U, [(0, 0)], widths, side)
    assert [int(v) for v in sums[:, 0]] == [(-1) ** w * U * M * M for w in widths]
    # beyond 2^32, still exact
    U, M, n = 3, 130, 33
    wide = np.repeat(random_tables(rng, 1, U, 1, n), M, axis=1)
    sums = gpu_ctx.shot_block_sums_host(wide, wide, U, [(0, 0)], [31, 32], side)
    assert [int(v) for v in sums[:, 0]] == [U * M * M * 2 ** 31, U * M * M * 2 ** 32] and int(sums[1, 0]) > 2 ** 32


def test_end_to_end_on_device_shots(gpu_ctx):
    c = END_TO_END
    U, M, n = c["settings"], c["shots_per_setting"], c["n"]
    states, B, host_bits = shot_case("end_to_end")
    assert np.array_equal(B, engine.setting_bases(8, 16, 12, c["shot_seed"]))
    pairs = upper_pairs(len(states))
    widths = np.arange(1, n + 1)
    with gpu_ctx.upload(states) as xs:
        bits = gpu_ctx.sample(xs, U * M, bases=B, seed=c["shot_seed"])
        assert np.array_equal(bits, host_bits)
        for side in SIDES:
            (O, Sx, _), (E, _, _) = gpu_ctx.shot_block_overlaps(bits, None, U, None, side, stderr=True)
            s, S = engine.shot_block_sums(host_bits, None, U, pairs, widths, side, per_setting=True)
            o, e = engine.shot_block_estimate(s, S, U, M, pairs[:, 0] == pairs[:, 1])
            assert np.array_equal(O[:, pairs[:, 1], pairs[:, 0]], o) and np.array_equal(E[:, pairs[:, 1], pairs[:, 0]], e)
            assert np.array_equal(O[:, np.arange(4), np.arange(4)], Sx)
            exact = gpu_ctx.block_overlaps(xs, None, None, side)[0]
            assert np.max(np.abs(exact[:, pairs[:, 1], pairs[:, 0]] - exact_block_overlaps(states, pairs, widths, side))) < 1e-12
            assert within_four_stderr(O, E, exact), side


def test_rejections(gpu_ctx):
    bx = random_tables(np.random.default_rng(12), 2, 2, 3, 5)
    for change, match in (
        (dict(pairs=[(0, 2)]), r"pairs\[0\]"),
        (dict(pairs=[(0, 1), (-1, 0)]), r"pairs\[1\]"),
        (dict(side=2), "side"),
        (dict(widths=[0, 1]), r"widths\[0\]"),
        (dict(widths=[2, 2]), r"widths\[1\]"),
        (dict(widths=[6]), r"widths\[0\]"),
        (dict(widths=[]), "n_widths"),
        (dict(pairs=[]), "n_pairs"),
        (dict(bits_x=bx + 2), "bits_x holds a bit other than 0 or 1"),
        (dict(bits_y=bx * 3), "bits_y holds a bit other than 0 or 1"),
        (dict(settings=6, pairs=[(1, 1)]), "shots_per_setting >= 2"),
    ):
        kw = {**dict(bits_x=bx, bits_y=None, settings=2, pairs=[(0, 1)], widths=[1, 5], side="left"), **change}
        with pytest.raises(engine.QkError, match=match):
            gpu_ctx.shot_block_sums_host(**kw)
    wide = random_tables(np.random.default_rng(13), 1, 1, 2, 40)
    with pytest.raises(engine.QkError, match=r"widths\[0\] = 33"):
        gpu_ctx.shot_block_sums_host(wide, None, 1, [(0, 0)], [33])
    # a bit outside the block's qubits is not read
    wide[0, 0, 39] = 7
    assert np.array_equal(gpu_ctx.shot_block_sums_host(wide, None, 1, [(0, 0)], [32]), engine.shot_block_sums(wide * (wide < 2), None, 1, [(0, 0)], [32]))
    with pytest.raises(engine.QkError, match="bits_x holds a bit"):
        gpu_ctx.shot_block_sums_host(wide, None, 1, [(0, 0)], [32], "right")
    # the overflow rule names its three numbers
    big = np.zeros((1, 2 ** 15 + 1, 32), dtype=np.uint8)
    with pytest.raises(engine.QkError, match=r"n_settings 1 x shots_per_setting 32769 \^2 x 2\^32"):
        gpu_ctx.shot_block_sums_host(big, None, 1, [(0, 0)], [32])
    # the raw entry point: null arguments and counts below 1
    L, h = engine.lib(), gpu_ctx.handle
    bits = np.ascontiguousarray(bx)
    pairs, widths, sums = np.zeros((1, 2), dtype=np.int32), np.ones(1, dtype=np.int32), np.zeros(1, dtype=np.int64)
    good = [h, 5, 2, 3, 2, bits.ctypes.data, 2, None, 1, pairs.ctypes.data, 0, 1, widths.ctypes.data, sums.ctypes.data, None]
    assert L.qk_shot_block_sums_host(*good) == 0
    for at, value, match in ((0, None, "ctx"), (5, None, "bits_x"), (9, None, "pairs"), (12, None, "widths"), (13, None, "sums"), (1, 0, "n_sites"), (2, 0, "n_settings"),
                             (3, 0, "shots_per_setting"), (4, 0, "nx"), (6, 0, "ny"), (6, 3, "ny 3 != nx 2"), (8, 0, "n_pairs"), (11, 0, "n_widths"), (10, -1, "side")):
        args = list(good)
        args[at] = value
        assert L.qk_shot_block_sums_host(*args) != 0
        assert match in L.qk_last_error().decode(), (at, L.qk_last_error())
    gpu_ctx.trim()  # the pair batch's scratch goes back; the next call takes it again
    assert np.array_equal(gpu_ctx.shot_block_sums_host(bx, None, 2, [(0, 1)], [1, 5]), engine.shot_block_sums(bx, None, 2, [(0, 1)], [1, 5]))


def _dist_inputs(Q_, R_):
    n = DIST["n"]
    ans = Q_.KernelStateAnsatz(n, DIST["layers"], 1.0, Q_.entanglement_graph(n, 2))
    return ans, R_.synthetic_features(DIST["nx"], n, 13), R_.synthetic_features(DIST["ny"], n, 14)


def _dist_runs(build, comm, ans, X, Y):
    kw = dict(widths=DIST["widths"], truncation_error=1e-16, shots=DIST["shots"], shot_seed=DIST["seed"])
    return {"train": build(comm, ans, X, side="left", form="rbf", **kw), "test": build(comm, ans, X, Y, side="right", form="overlap", **kw)}


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
        from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_block_kernel_matrices

        q.put((rank, _dist_runs(build_block_kernel_matrices, TorchComm(), *_dist_inputs(Q_, R_))))
    finally:
        dist.destroy_process_group()


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.timeout(300)
def test_two_ranks_match_one_rank_bitwise(built, monkeypatch):
    import torch.multiprocessing as mp

    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_block_kernel_matrices

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + ((os.getpid() + 1511) % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert res[1]["train"] is None and res[1]["test"] is None
    monkeypatch.setenv("QK_BUILDER", "host")
    one = _dist_runs(build_block_kernel_matrices, SingleComm(), *_dist_inputs(Q, R))
    for which in ("train", "test"):
        assert _same(res[0][which], one[which]), which


def test_build_block_kernel_matrices_with_shots(built, gpu_ctx, monkeypatch):
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_block_kernel_matrices

    monkeypatch.setenv("QK_BUILDER", "host")
    ans, X, Y = _dist_inputs(Q, R)
    n, (U, M), seed, widths = DIST["n"], DIST["shots"], DIST["seed"], list(DIST["widths"])
    out = _dist_runs(build_block_kernel_matrices, SingleComm(), ans, X, Y)
    # against the pieces: the states of Y are sampled with indices after those of X, every state in the same bases
    xs = [Q.simulate(ans.circuit_for_data(x), 1 - 1e-16) for x in X]
    ys = [Q.simulate(ans.circuit_for_data(y), 1 - 1e-16) for y in Y]
    B = engine.setting_bases(U, M, n, seed)
    bx = np.stack([m.sample(U * M, bases=B, seed=seed, state_index=s) for s, m in enumerate(xs)])
    by = np.stack([m.sample(U * M, bases=B, seed=seed, state_index=len(xs) + s) for s, m in enumerate(ys)])
    tr, te = out["train"], out["test"]
    assert tr["shots"] == (U, M) and tr["widths"] == widths
    (O, Sx, _), (E, Ex, _) = gpu_ctx.shot_block_overlaps(bx, None, U, widths, "left", stderr=True)
    for wi, w in enumerate(widths):
        assert np.array_equal(tr["overlap"][w], O[wi]) and np.array_equal(tr["stderr"]["overlap"][w], E[wi])
        assert np.array_equal(tr["K"][w], engine.block_kernel(O[wi], Sx[wi], form="rbf"))
    assert np.array_equal(tr["self_x"], Sx) and tr["self_y"] is tr["self_x"] and np.array_equal(tr["stderr"]["self_x"], Ex)
    (O, Sx, Sy), (E, Ex, Ey) = gpu_ctx.shot_block_overlaps(bx, by, U, widths, "right", stderr=True)
    for wi, w in enumerate(widths):
        assert np.array_equal(te["overlap"][w], O[wi]) and np.array_equal(te["K"][w], O[wi]) and np.array_equal(te["stderr"]["overlap"][w], E[wi])
    assert np.array_equal(te["self_x"], Sx) and np.array_equal(te["self_y"], Sy)
    assert np.array_equal(te["stderr"]["self_x"], Ex) and np.array_equal(te["stderr"]["self_y"], Ey)
    # shots=None returns what it returned before: the exact family, without the new keys
    exact = build_block_kernel_matrices(SingleComm(), ans, X, Y, widths=widths, side="right", form="overlap", truncation_error=1e-16)
    assert sorted(exact) == ["K", "overlap", "self_x", "self_y", "widths"]
    with gpu_ctx.upload(xs) as sx, gpu_ctx.upload(ys) as sy:
        O_exact, Sx_exact, Sy_exact = gpu_ctx.block_overlaps(sx, sy, widths, "right")
    for wi, w in enumerate(widths):
        assert np.array_equal(exact["overlap"][w], O_exact[wi])
    assert np.array_equal(exact["self_x"], Sx_exact) and np.array_equal(exact["self_y"], Sy_exact)
    # and the estimates are estimates of it
    assert np.max(np.abs(te["overlap"][1] - exact["overlap"][1])) < 0.5
    for kwargs, match in ((dict(shots=(8, 16), widths=[33]), "widths"), (dict(shots=8), "shots"), (dict(shots=(0, 4)), "shots"), (dict(shots=(4, 1)), "shots_per_setting")):
        with pytest.raises(ValueError, match=match):
            build_block_kernel_matrices(SingleComm(), ans, X, truncation_error=1e-16, **kwargs)
