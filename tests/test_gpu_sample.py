"""Measurement shots on the MI355X: qk_sample_host against the host mirror ``MPS.sample`` on identical tensors -- the log probability
of every drawn string to 1e-11 and, where no draw of the mirror sits on a threshold, the bits exactly --, against the Born
probability of the dense state vector, general-gauge states with bonds up to 300 (dense complex R_k, several column blocks),
circuits whose outcomes are certain, the bit guarantees (a state alone, the cut into chain batches, fewer shots, two runs, a device-
built set), the rejections, and ``build_projected_kernel_matrix(shots=...)`` against the pipeline spelled out by hand, on one rank
and on two."""
import functools
import os
import sys

import numpy as np
import pytest

import qml_cutensornet_amd as Q
from helpers import GAUGE_SAMPLE, SHOTS, gauge_sample_case, gauge_set_300, gauge_sets
from oracle import restatement as R
from qml_cutensornet_amd import engine
from test_sample_host import ansatz_states, dense_of_mps, dense_probability

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (states, bases (SHOTS, n), seed).  The seeds were chosen on the CPU so that no draw of the host mirror sits within
    1e-9 of its threshold (test_bits_equal_the_mirror asserts it): the smallest margin of these draws is about 1e-4.

    "g20" and "g300" are the general-gauge cases of tests/helpers.py: states whose R_k is dense and complex at every bond, which the
    canonical ones above never give the sampler (their R_k is the identity or a real diagonal), on bonds that make SMP_Q take several
    column blocks and the draw loop run more than once (test_general_gauge_cases_cross_the_blocks)."""
    a12, _ = ansatz_states(12, 3, 6, 1)
    a12 = [a12[i] for i in (0, 1, 2, 5)]  # largest bonds 50, 30, 41, 50: no multiple of 16, both sides of 48
    a9, _ = ansatz_states(9, 2, 3, 21)
    rng = np.random.default_rng(12)
    two = [Q.random_mps(2, [1, 2, 1], rng) for _ in range(3)]
    one = [Q.random_mps(1, [1, 1], rng) for _ in range(2)]
    gauge = {name: gauge_sample_case(name)[:3] for name in GAUGE_SAMPLE}
    return {**gauge, "a12": (a12, engine.random_bases(SHOTS, 12, 41), 7), "a9": (a9, engine.random_bases(SHOTS, 9, 42), 8),
            "two": (two, engine.random_bases(SHOTS, 2, 43), 2**40 + 9), "one": (one, engine.random_bases(SHOTS, 1, 44), 10)}


@functools.lru_cache(maxsize=None)
def mirror(name):
    """(bits, logp, margin) of the host mirror for every state of a case, state i with global index i."""
    states, bases, seed = cases()[name]
    out = [m.sample(SHOTS, bases=bases, seed=seed, state_index=i, logp=True, margin=True) for i, m in enumerate(states)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), [o[2] for o in out]


@pytest.fixture(scope="module")
def device(gpu_ctx):
    """name -> (bits, logp) of the device for every case, one call each."""
    out = {}
    for name, (states, bases, seed) in cases().items():
        with gpu_ctx.upload(states) as xs:
            out[name] = gpu_ctx.sample(xs, SHOTS, bases=bases, seed=seed, logp=True)
    return out


NAMES = ["a12", "a9", "two", "one", "g20", "g300"]


@pytest.mark.parametrize("name", NAMES)
def test_logp_against_the_mirror_and_the_dense_vector(device, name):
    states, bases, _ = cases()[name]
    bits, lp = device[name]
    n = len(states[0])
    assert bits.shape == (len(states), SHOTS, n) and bits.dtype == np.uint8 and bits.max() <= 1 and lp.shape == (len(states), SHOTS)
    if name == "a12":
        assert sorted(m.max_bond() for m in states) == [30, 41, 50, 50]
    hbits, hlp, _ = mirror(name)
    print(f"{name}: max |logp_hip - logp_mirror| = {np.abs(lp - hlp).max():.3e} over {lp.size} shots, {int((bits != hbits).sum())} bits differ")
    assert np.abs(lp - hlp).max() <= 1e-11
    if n > 18:  # the dense checks stay at 18 qubits or fewer
        return
    for i, m in enumerate(states):
        exact = dense_probability(dense_of_mps(m), bits[i], bases)
        assert np.all(np.abs(np.exp(lp[i]) - exact) <= 1e-8 * exact)


@pytest.mark.parametrize("name", NAMES)
def test_bits_equal_the_mirror(device, name):
    hbits, _, margins = mirror(name)
    # a condition on the inputs, not a tolerance: no draw of the mirror is closer than 1e-9 to its threshold
    assert min(margins) >= 1e-9, margins
    assert np.array_equal(device[name][0], hbits)


def test_general_gauge_cases_cross_the_blocks(gpu_ctx):
    """From the sets' own bond tables: padded bonds of 64, 80 and of 128 or more ("g300": 304), so SMP_Q has two to five column
    blocks, SMP_W up to ten, and the 64-wide loops of the draw kernel run more than once."""
    for name, want in (("g20", (64, 80, 128)), ("g300", (64, 128, 208, 304))):
        with gpu_ctx.upload(cases()[name][0]) as xs:
            pads = set(((np.asarray(xs.dims) + 15) // 16 * 16).ravel().tolist())
        assert all(w in pads for w in want), (name, sorted(pads))
        assert max(pads) >= 128


@pytest.mark.parametrize("name", list(GAUGE_SAMPLE))
def test_general_gauge_twins_draw_their_originals_bits(gpu_ctx, device, name):
    """A twin and its right-orthonormal original are one state, and under equal global indices they take equal uniforms: equal
    bits (no draw of either mirror is within 1e-9 of its threshold: tests/test_gauge_inputs_host.py) and |d logp| <= 1e-11, the bound
    of the device against its mirror (the mirrors of the two drift by 3e-14).  Measured on the MI355X: |d logp| = 2.3e-14 ("g20") and
    4.3e-14 ("g300"); against the mirror the two cases are at 2.5e-14 and 3.2e-14, no bit differs."""
    _, bases, seed, first = gauge_sample_case(name)
    originals = list((gauge_sets if name == "g20" else gauge_set_300)()[0])
    with gpu_ctx.upload(originals) as xs:
        bits, lp = gpu_ctx.sample(xs, SHOTS, bases=bases, seed=seed, first_state=first, logp=True)
    tb, tl = device[name][0][first:], device[name][1][first:]
    print(f"{name}: twin vs original on the device: {int((bits != tb).sum())} bits differ, max |d logp| = {np.abs(lp - tl).max():.3e}")
    assert np.array_equal(bits, tb)
    assert np.abs(lp - tl).max() <= 1e-11


def test_general_gauge_batches_of_one_chain(gpu_ctx, device, monkeypatch):
    states, bases, seed = cases()["g20"]
    monkeypatch.setenv("QK_SAMPLE_BATCH", "1")  # 12 chains, one per batch
    with gpu_ctx.upload(states) as xs:
        bits, lp = gpu_ctx.sample(xs, SHOTS, bases=bases, seed=seed, logp=True)
    assert np.array_equal(bits, device["g20"][0]) and np.array_equal(lp, device["g20"][1])


def test_one_shot(gpu_ctx, device):
    states, bases, seed = cases()["a12"]
    with gpu_ctx.upload(states) as xs:
        bits, lp = gpu_ctx.sample(xs, 1, bases=bases[:1], seed=seed, logp=True)
    assert bits.shape == (4, 1, 12)
    assert np.array_equal(bits, device["a12"][0][:, :1]) and np.array_equal(lp, device["a12"][1][:, :1])
    # without logp the result is the bits alone; None is all Z
    with gpu_ctx.upload(states[:1]) as xs:
        z = gpu_ctx.sample(xs, 3, seed=5)
        assert isinstance(z, np.ndarray) and np.array_equal(z, gpu_ctx.sample(xs, 3, bases="Z" * 12, seed=5))
        assert np.array_equal(z[0], states[0].sample(3, seed=5))


def test_certain_outcomes(gpu_ctx):
    n = 5
    plus = Q.simulate(Q.BoundCircuit.from_gates(n, [("H", [q], []) for q in range(n)]), 1 - 1e-16)
    with gpu_ctx.upload([plus]) as xs:
        bits, lp = gpu_ctx.sample(xs, 40, bases="X" * n, seed=1, logp=True)
    assert not bits.any() and np.abs(lp).max() < 1e-12
    bell = Q.simulate(Q.BoundCircuit.from_gates(2, [("XXPhase", [0, 1], [0.5])]), 1 - 1e-16)
    with gpu_ctx.upload([bell]) as xs:
        bits, lp = gpu_ctx.sample(xs, 200, seed=4, logp=True)
    assert np.array_equal(bits[0, :, 0], bits[0, :, 1]) and 0 < bits[0, :, 0].sum() < 200
    assert np.abs(np.exp(lp) - 0.5).max() < 1e-12
    states, _ = ansatz_states(8, 2, 2, 5, hadamard_init=False)
    with gpu_ctx.upload(states) as xs:
        bits = gpu_ctx.sample(xs, 100, seed=9)
    assert not (bits.sum(axis=2) % 2).any() and bits.any()
    alphas = (0.3, 0.5, 1.2)
    rys = [Q.simulate(Q.BoundCircuit.from_gates(1, [("Ry", [0], [a])]), 1 - 1e-16) for a in alphas]
    with gpu_ctx.upload(rys) as xs:
        bits, lp = gpu_ctx.sample(xs, 50, seed=3, logp=True)
    for i, a in enumerate(alphas):
        want = np.where(bits[i, :, 0] == 0, np.cos(np.pi * a / 2) ** 2, np.sin(np.pi * a / 2) ** 2)
        assert len(np.unique(bits[i])) == 2 and np.abs(np.exp(lp[i]) - want).max() < 1e-12


def test_bit_guarantees(gpu_ctx, device, monkeypatch):
    states, bases, seed = cases()["a12"]
    bits, lp = device["a12"]
    for i in (1, 3):  # a state alone, with its global index
        with gpu_ctx.upload([states[i]]) as xs:
            b1, l1 = gpu_ctx.sample(xs, SHOTS, bases=bases, seed=seed, first_state=i, logp=True)
        assert np.array_equal(b1[0], bits[i]) and np.array_equal(l1[0], lp[i])
    with gpu_ctx.upload(states) as xs:
        for cap in ("1", "3"):  # 8 chains in batches of one and of three
            monkeypatch.setenv("QK_SAMPLE_BATCH", cap)
            bc, lc = gpu_ctx.sample(xs, SHOTS, bases=bases, seed=seed, logp=True)
            assert np.array_equal(bc, bits) and np.array_equal(lc, lp)
        monkeypatch.setenv("QK_SAMPLE_BATCH", "0")
        with pytest.raises(engine.QkError, match="QK_SAMPLE_BATCH"):
            gpu_ctx.sample(xs, 2)
        monkeypatch.delenv("QK_SAMPLE_BATCH")
        b17, l17 = gpu_ctx.sample(xs, 17, bases=bases[:17], seed=seed, logp=True)  # fewer shots: the head of the longer call
        assert np.array_equal(b17, bits[:, :17]) and np.array_equal(l17, lp[:, :17])
        again = gpu_ctx.sample(xs, SHOTS, bases=bases, seed=seed, logp=True)  # two runs
        assert np.array_equal(again[0], bits) and np.array_equal(again[1], lp)
        other = gpu_ctx.sample(xs, SHOTS, bases=bases, seed=seed + 1)
        assert not np.array_equal(other, bits)
    # a set built on the device and the same tensors uploaded
    ans = Q.KernelStateAnsatz(9, 2, 1.0, Q.entanglement_graph(9, 2))
    circs = [ans.circuit_for_data(x) for x in R.synthetic_features(4, 9, 6)]
    b9 = engine.random_bases(SHOTS, 9, 3)
    built, _ = gpu_ctx.build_mps_set(circs)
    with built:
        tensors = built.download()
        on_device = gpu_ctx.sample(built, SHOTS, bases=b9, seed=11, logp=True)
    with gpu_ctx.upload(tensors) as xs:
        uploaded = gpu_ctx.sample(xs, SHOTS, bases=b9, seed=11, logp=True)
    assert np.array_equal(on_device[0], uploaded[0]) and np.array_equal(on_device[1], uploaded[1])


def test_rejections(gpu_ctx):
    states, bases, _ = cases()["a9"]
    with gpu_ctx.upload(states) as xs:
        with xs.to_f32() as x32:
            with pytest.raises(engine.QkError, match="set is complex64"):
                gpu_ctx.sample(x32, 4)
        with pytest.raises(engine.QkError, match="n_shots"):
            gpu_ctx.sample(xs, 0)
        for code in (0, 4):
            bad = bases[:8].copy()
            bad[5, 3] = code
            with pytest.raises(engine.QkError, match=rf"bases\[5\]\[3\] = {code}"):
                gpu_ctx.sample(xs, 8, bases=bad)
        for wrong in (bases[:7], bases[:8, :8], np.ones((8, 9)), "ZZZ"):
            with pytest.raises(ValueError, match="bases"):
                gpu_ctx.sample(xs, 8, bases=wrong)
        with pytest.raises(ValueError, match="shots"):
            gpu_ctx.sample(xs, 2.5)
        with pytest.raises(engine.QkError, match="first_state"):
            gpu_ctx.sample(xs, 2, first_state=-1)
        # a state of norm 0 is named
        zero = Q.MPS([0.0 * t for t in states[1].tensors])
    with gpu_ctx.upload([states[0], zero]) as xs:
        with pytest.raises(engine.QkError, match="state 1"):
            gpu_ctx.sample(xs, 4)


def _by_hand(ctx, ans, X, Y, shots, seed, rdm, D):
    """Context.sample, the estimators and the projected Gram, on the sets the builder of the call makes."""
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import _simulate_share

    n = int(ans.num_qubits)
    bases = engine.random_bases(shots, n, seed)
    feats = []
    for label, pts, first in (("X", X, 0), ("Y", Y, len(X))):
        if pts is None:
            continue
        _, xs, _, _ = _simulate_share(ans, np.asarray(pts, dtype=np.float64), 0, 1, 1 - 1e-16, False, label)
        bits = ctx.sample(xs, shots, bases=bases, seed=seed, first_state=first)
        xs.close()
        feats.append(engine.estimate_paulis(bits, bases)[0] if rdm == 1 else engine.estimate_pair_paulis(bits, bases, D))
    fy = None if Y is None else feats[1]
    return ctx.projected_gram(feats[0], fy) if rdm == 1 else ctx.projected_pair_gram(feats[0], fy, max_dist=D)


E2E = dict(n=10, layers=2, nx=9, ny=5, shots=256, seed=77)


def test_build_projected_kernel_matrix_with_shots(gpu_ctx, monkeypatch, tmp_path):
    import json

    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_projected_kernel_matrix

    monkeypatch.setenv("QK_BUILDER", "host")
    n, S, seed = E2E["n"], E2E["shots"], E2E["seed"]
    ans = Q.KernelStateAnsatz(n, E2E["layers"], 1.0, Q.entanglement_graph(n, 2))
    X, Y = R.synthetic_features(E2E["nx"], n, 13), R.synthetic_features(E2E["ny"], n, 14)
    ctx = engine.default_context(0)
    info = str(tmp_path / "prof")
    for kwargs in (dict(rdm=1), dict(rdm=2, pair_distance=2)):
        K = build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, shots=S, shot_seed=seed, info_file=info, **kwargs)
        assert json.load(open(info + ".json"))["pqk_shots"][0] == S
        hand = _by_hand(ctx, ans, X, None, S, seed, kwargs["rdm"], kwargs.get("pair_distance", 1))
        assert K.shape == (E2E["nx"], E2E["nx"]) and np.array_equal(K, hand)
        assert np.array_equal(K, K.T) and np.all(np.diag(K) == 1.0)
        exact = build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, **kwargs)
        assert np.array_equal(exact, build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, shots=None, **kwargs))
        assert 1e-4 < np.abs(K - exact).max() < 0.5  # shot noise: another matrix, not a far one
        Kt = build_projected_kernel_matrix(SingleComm(), ans, X, Y=Y, truncation_error=1e-16, shots=S, shot_seed=seed, **kwargs)
        assert Kt.shape == (E2E["ny"], E2E["nx"]) and np.array_equal(Kt, _by_hand(ctx, ans, X, Y, S, seed, kwargs["rdm"], kwargs.get("pair_distance", 1)))
    # shots=None is today's call: the exact Bloch vectors
    with ctx.upload([Q.simulate(ans.circuit_for_data(x), 1 - 1e-16) for x in X]) as xs:
        assert np.array_equal(build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16), ctx.projected_gram(ctx.local_paulis(xs)))
    with pytest.raises(ValueError, match="observables"):
        build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, shots=S, observables=["Z" * n])
    with pytest.raises(ValueError, match="shots"):
        build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, shots=0)


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
        from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_projected_kernel_matrix

        n, S, seed = E2E["n"], E2E["shots"], E2E["seed"]
        ans = Q_.KernelStateAnsatz(n, E2E["layers"], 1.0, Q_.entanglement_graph(n, 2))
        X, Y = R_.synthetic_features(E2E["nx"], n, 13), R_.synthetic_features(E2E["ny"], n, 14)
        comm = TorchComm()
        out = {"train": build_projected_kernel_matrix(comm, ans, X, truncation_error=1e-16, shots=S, shot_seed=seed, rdm=1),
               "test": build_projected_kernel_matrix(comm, ans, X, Y=Y, truncation_error=1e-16, shots=S, shot_seed=seed, rdm=2, pair_distance=2)}
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_match_one_rank_bitwise(built, monkeypatch):
    import torch.multiprocessing as mp

    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_projected_kernel_matrix

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + ((os.getpid() + 977) % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert res[1]["train"] is None and res[1]["test"] is None
    monkeypatch.setenv("QK_BUILDER", "host")
    n, S, seed = E2E["n"], E2E["shots"], E2E["seed"]
    ans = Q.KernelStateAnsatz(n, E2E["layers"], 1.0, Q.entanglement_graph(n, 2))
    X, Y = R.synthetic_features(E2E["nx"], n, 13), R.synthetic_features(E2E["ny"], n, 14)
    one = build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, shots=S, shot_seed=seed, rdm=1)
    one_t = build_projected_kernel_matrix(SingleComm(), ans, X, Y=Y, truncation_error=1e-16, shots=S, shot_seed=seed, rdm=2, pair_distance=2)
    assert np.array_equal(res[0]["train"], one)
    assert np.array_equal(res[0]["test"], one_t)
