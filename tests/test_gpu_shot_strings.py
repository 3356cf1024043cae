"""GPU tier: Pauli strings and window RDMs estimated from measurement shots on the MI355X (qk_shot_strings_host,
Context.shot_string_sums_host / estimate_pauli_strings / estimate_window_rdms, build_shot_feature_kernel_matrix).  Everything is integer
arithmetic, so every case is ``np.array_equal`` against the numpy mirror ``engine.shot_string_sums``: random tables at the qubit
counts where a group begins or ends and the shot and string counts where a chunk or a block does, the cut invariances, real shots
of ansatz states against the older estimators, the rejections, and the builder against its pieces on one rank and on two."""
import os
import sys

import numpy as np
import pytest

import qml_cutensornet_amd as Q
from oracle import restatement as R
from qml_cutensornet_amd import engine
from test_pauli_strings_host import pair_strings, weight_one_strings
from test_sample_host import ansatz_states
from test_shot_strings_host import random_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, shots, strings, states, per-state bases): every n, shots and strings of the lists below appears, ragged against the 32 qubits of
# a group, the 256 shots of a chunk (and the four waves that share it) and the 64 strings of a block
TABLES = [(1, 1, 1, 1, False), (31, 63, 63, 2, True), (32, 64, 64, 3, False), (33, 65, 65, 5, True), (64, 257, 130, 2, False), (65, 64, 130, 4, True),
          (96, 257, 65, 1, True), (128, 65, 63, 3, False), (128, 257, 1, 2, True), (1, 257, 64, 5, False)]


@pytest.mark.parametrize("n,shots,m,ns,per_state", TABLES)
def test_device_equals_mirror(gpu_ctx, n, shots, m, ns, per_state):
    rng = np.random.default_rng(7 * n + shots + m)
    bits, bases, S = random_case(rng, ns, shots, n, m, per_state)
    sums, counts = gpu_ctx.shot_string_sums_host(bits, bases, S)
    want_s, want_c = engine.shot_string_sums(bits, bases, S)
    assert sums.dtype == np.int64 and counts.dtype == np.int64 and sums.shape == (ns, m)
    assert np.array_equal(sums, want_s) and np.array_equal(counts, want_c)
    assert np.all(counts[:, 0] == shots) and np.all(sums[:, 0] == shots)  # the identity
    if m > 1:
        assert counts[0, 1] >= 1 and (S[1] != 0).all()  # the full-weight string matches the shot it was copied from


def test_cut_invariance(gpu_ctx, monkeypatch):
    rng = np.random.default_rng(3)
    bits, bases, S = random_case(rng, 4, 300, 40, 130, True)
    monkeypatch.delenv("QK_SHOT_STRINGS_BATCH", raising=False)
    sums, counts = gpu_ctx.shot_string_sums_host(bits, bases, S)
    assert np.array_equal(sums, engine.shot_string_sums(bits, bases, S)[0])
    for cap in ("1", "7"):
        monkeypatch.setenv("QK_SHOT_STRINGS_BATCH", cap)
        s, c = gpu_ctx.shot_string_sums_host(bits, bases, S)
        assert np.array_equal(s, sums) and np.array_equal(c, counts)
    monkeypatch.setenv("QK_SHOT_STRINGS_BATCH", "0")
    with pytest.raises(engine.QkError, match="QK_SHOT_STRINGS_BATCH"):
        gpu_ctx.shot_string_sums_host(bits, bases, S)
    monkeypatch.delenv("QK_SHOT_STRINGS_BATCH")
    s1, c1 = gpu_ctx.shot_string_sums_host(bits[2:3], bases[2:3], S)  # a state alone
    assert np.array_equal(s1[0], sums[2]) and np.array_equal(c1[0], counts[2])
    cols = rng.permutation(130)[:71]  # a subset of the strings, in another order
    s2, c2 = gpu_ctx.shot_string_sums_host(bits, bases, S[cols])
    assert np.array_equal(s2, sums[:, cols]) and np.array_equal(c2, counts[:, cols])
    s3, c3 = gpu_ctx.shot_string_sums_host(bits, bases, S)  # two runs
    assert np.array_equal(s3, sums) and np.array_equal(c3, counts)
    gpu_ctx.trim()  # the scratch goes back, and comes again
    s4, _ = gpu_ctx.shot_string_sums_host(bits, bases, S)
    assert np.array_equal(s4, sums)


def test_real_shots_end_to_end(gpu_ctx):
    n, shots = 8, 512
    states, _ = ansatz_states(n, 2, 3, 9)
    bases = engine.random_bases(shots, n, 4)
    with gpu_ctx.upload(states) as xs:
        bits = gpu_ctx.sample(xs, shots, bases=bases, seed=6)
    V, counts = gpu_ctx.estimate_pauli_strings(bits, bases, weight_one_strings(n))
    F, fc = engine.estimate_paulis(bits, bases)
    assert np.array_equal(V.reshape(3, n, 3), F) and np.array_equal(counts[0].reshape(n, 3), fc)
    V2, _ = gpu_ctx.estimate_pauli_strings(bits, bases, pair_strings(n, 2))
    assert np.array_equal(V2.reshape(3, -1, 4, 4), engine.estimate_pair_paulis(bits, bases, max_dist=2))
    for width in (1, 2, 3):
        rho, cnt = gpu_ctx.estimate_window_rdms(bits, bases, width)
        want, want_c = engine.estimate_window_rdms(bits, bases, width)
        assert rho.shape == (3, n - width + 1, 1 << width, 1 << width) and np.array_equal(rho, want) and np.array_equal(cnt, want_c)
        assert np.array_equal(rho, np.conj(np.swapaxes(rho, -1, -2)))
    some, _ = gpu_ctx.estimate_window_rdms(bits, bases, 3, starts=[0, 4])
    assert np.array_equal(some, engine.estimate_window_rdms(bits, bases, 3)[0][:, [0, 4]])
    # circuits without the Hadamard layer conserve parity: Z on every qubit is +1 in every shot
    even, _ = ansatz_states(n, 2, 2, 5, hadamard_init=False)
    with gpu_ctx.upload(even) as xs:
        zbits = gpu_ctx.sample(xs, 100, seed=9)
    vals, cz = gpu_ctx.estimate_pauli_strings(zbits, np.full((100, n), 3, dtype=np.uint8), ["Z" * n, "Z" + "I" * (n - 1)])
    assert np.all(vals[:, 0] == 1.0) and np.all(cz == 100) and zbits.any()


def test_rejections(gpu_ctx):
    L = engine.lib()
    n, ns, T, m = 3, 2, 4, 2
    bits = np.zeros((ns, T, n), dtype=np.uint8)
    bases = np.full((T, n), 3, dtype=np.uint8)
    S = np.array([[0, 1, 2], [3, 0, 0]], dtype=np.uint8)
    sums, counts = np.zeros((ns, m), dtype=np.int64), np.zeros((ns, m), dtype=np.int64)
    h = gpu_ctx.handle
    good = [h, n, ns, T, bits.ctypes.data, bases.ctypes.data, 0, m, S.ctypes.data, sums.ctypes.data, counts.ctypes.data]
    assert L.qk_shot_strings_host(*good) == 0 and np.array_equal(counts, [[0, 4], [0, 4]]) and np.array_equal(sums, counts)
    for at, value, name in ((0, None, "ctx"), (4, None, "bits"), (5, None, "bases"), (8, None, "strings"), (9, None, "sums"), (10, None, "counts"), (1, 0, "n_sites"),
                            (1, 129, "n_sites"), (2, 0, "n_states"), (3, 0, "shots"), (7, 0, "n_strings"), (6, 2, "bases_per_state"), (6, -1, "bases_per_state")):
        args = list(good)
        args[at] = value
        assert L.qk_shot_strings_host(*args) != 0
        assert name in L.qk_last_error().decode(), (name, L.qk_last_error().decode())
    bad = bits.copy()
    bad[1, 2, 1] = 2
    with pytest.raises(engine.QkError, match="bits"):
        gpu_ctx.shot_string_sums_host(bad, bases, S)
    for code in (0, 4):
        wrong = bases.copy()
        wrong[3, 0] = code
        with pytest.raises(engine.QkError, match="bases"):
            gpu_ctx.shot_string_sums_host(bits, wrong, S)
        with pytest.raises(engine.QkError, match="bases"):
            gpu_ctx.shot_string_sums_host(bits, np.stack([bases, wrong]), S)
    with pytest.raises(engine.QkError, match=r"strings\[1\]"):
        gpu_ctx.shot_string_sums_host(bits, bases, np.array([[0, 1, 2], [0, 4, 0]], dtype=np.uint8))
    with pytest.raises(ValueError, match="bases"):
        gpu_ctx.shot_string_sums_host(bits, bases[:3], S)
    with pytest.raises(ValueError, match="width"):
        gpu_ctx.estimate_window_rdms(bits, bases, 4)
    # the call after a rejection is whole
    assert np.array_equal(gpu_ctx.shot_string_sums_host(bits, bases, S)[1], [[0, 4], [0, 4]])


# strings of weight 1 to 3: at 270 shots in random bases a string of weight v is seen by about 270 / 3^v shots, so heavier ones are noise alone
E2E = dict(n=10, layers=2, nx=9, ny=5, shots=270, seed=77, observables=[("ZZZ", (0, 1, 2)), ("XX", (0, 1)), ("YZY", (3, 4, 5)), ("ZZ", (2, 9)), ("XY", (5, 8)), ("Z", (7,))],
           window=3)


def _inputs(Q_, R_):
    n = E2E["n"]
    ans = Q_.KernelStateAnsatz(n, E2E["layers"], 1.0, Q_.entanglement_graph(n, 2))
    return ans, R_.synthetic_features(E2E["nx"], n, 13), R_.synthetic_features(E2E["ny"], n, 14)


FORMS = {"observables": dict(observables=E2E["observables"]), "window": dict(window=E2E["window"]), "designed": dict(window=E2E["window"], settings="window")}


def _by_hand(ctx, ans, X, Y, form):
    """Context.sample, the estimators and the Gram, on the sets the builder of the call makes."""
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import _simulate_share

    n, shots, seed = int(ans.num_qubits), E2E["shots"], E2E["seed"]
    bases = engine.window_settings(shots, n, E2E["window"]) if form == "designed" else engine.random_bases(shots, n, seed)
    feats = []
    for label, pts, first in (("X", X, 0), ("Y", Y, len(X))):
        if pts is None:
            continue
        _, xs, _, _ = _simulate_share(ans, np.asarray(pts, dtype=np.float64), 0, 1, 1 - 1e-16, False, label)
        bits = ctx.sample(xs, shots, bases=bases, seed=seed, first_state=first)
        xs.close()
        if form == "observables":
            feats.append(ctx.estimate_pauli_strings(bits, bases, E2E["observables"])[0])
        else:
            feats.append(ctx.estimate_window_rdms(bits, bases, E2E["window"])[0])
    fy = None if Y is None else feats[1]
    return ctx.feature_gram(feats[0], fy) if form == "observables" else ctx.projected_window_gram(feats[0], fy)


@pytest.mark.parametrize("form", list(FORMS))
def test_build_shot_feature_kernel_matrix_against_its_pieces(gpu_ctx, monkeypatch, tmp_path, form):
    import json

    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_projected_kernel_matrix, build_shot_feature_kernel_matrix

    monkeypatch.setenv("QK_BUILDER", "host")
    ans, X, Y = _inputs(Q, R)
    ctx = engine.default_context(0)
    info = str(tmp_path / "prof")
    kw = dict(truncation_error=1e-16, shots=E2E["shots"], shot_seed=E2E["seed"], **FORMS[form])
    K = build_shot_feature_kernel_matrix(SingleComm(), ans, X, info_file=info, **kw)
    prof = json.load(open(info + ".json"))
    assert prof["pqk_shots"][0] == E2E["shots"]
    if form == "observables":
        assert prof["pqk_observables"][0] == len(E2E["observables"]) and "pqk_rdm" not in prof and prof["pqk_gamma"][0] == 1.0 / len(E2E["observables"])
        exact = build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, observables=E2E["observables"])
    else:
        assert prof["pqk_rdm"][0] == E2E["window"] and "pqk_observables" not in prof and prof["pqk_gamma"][0] == 1.0 / E2E["n"]
        exact = build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, rdm=E2E["window"], window=True)
    assert K.shape == (E2E["nx"], E2E["nx"]) and np.array_equal(K, _by_hand(ctx, ans, X, None, form))
    assert np.array_equal(K, K.T) and np.all(np.diag(K) == 1.0)
    print(f"{form}: max |K - K_exact| = {np.abs(K - exact).max():.3e}")
    assert 1e-4 < np.abs(K - exact).max() < 0.5  # shot noise: another matrix, not a far one
    Kt = build_shot_feature_kernel_matrix(SingleComm(), ans, X, Y=Y, **kw)
    assert Kt.shape == (E2E["ny"], E2E["nx"]) and np.array_equal(Kt, _by_hand(ctx, ans, X, Y, form))


@pytest.mark.parametrize(
    "kwargs,match",
    [
        (dict(observables=["Z" * 10], window=3, shots=8), "exactly one"),
        (dict(shots=8), "exactly one"),
        (dict(window=3, shots=0), "shots"),
        (dict(window=3), "shots"),
        (dict(window=3, shots=True), "shots"),
        (dict(observables=["Z" * 10], shots=8, settings="window"), "settings"),
        (dict(window=3, shots=26, settings="window"), "3\\^window"),
        (dict(window=3, shots=8, settings="designed"), "settings"),
        (dict(window=0, shots=8), "window"),
        (dict(window=7, shots=8), "window"),
        (dict(window=True, shots=8), "window"),
        (dict(observables=["ZZ"], shots=8), "ZZ"),
        (dict(observables=[], shots=8), "empty"),
        (dict(window=3, shots=8, pqk_gamma=0.0), "bandwidth"),
    ],
)
def test_build_shot_feature_kernel_matrix_argument_errors(monkeypatch, kwargs, match):
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_shot_feature_kernel_matrix

    def no_device(*a, **k):
        raise AssertionError("device work before the argument checks")

    monkeypatch.setattr(engine, "device_count", no_device)
    monkeypatch.setattr(engine, "default_context", no_device)
    ans, X, _ = _inputs(Q, R)
    with pytest.raises(ValueError, match=match):
        build_shot_feature_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, **kwargs)


def _runs(build, comm, ans, X, Y):
    kw = dict(truncation_error=1e-16, shots=E2E["shots"], shot_seed=E2E["seed"])
    return {"train": build(comm, ans, X, **kw, **FORMS["observables"]), "test": build(comm, ans, X, Y=Y, **kw, **FORMS["window"])}


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
        from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_shot_feature_kernel_matrix

        q.put((rank, _runs(build_shot_feature_kernel_matrix, TorchComm(), *_inputs(Q_, R_))))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_match_one_rank_bitwise(built, monkeypatch):
    import torch.multiprocessing as mp

    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_shot_feature_kernel_matrix

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + ((os.getpid() + 1531) % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert res[1]["train"] is None and res[1]["test"] is None
    monkeypatch.setenv("QK_BUILDER", "host")
    one = _runs(build_shot_feature_kernel_matrix, SingleComm(), *_inputs(Q, R))
    assert np.array_equal(res[0]["train"], one["train"])
    assert np.array_equal(res[0]["test"], one["test"])
