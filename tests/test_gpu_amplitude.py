"""Amplitudes of given strings on the MI355X: qk_amplitudes_host against the host mirror ``MPS.amplitude`` on identical tensors -- every
amplitude to 1e-11 relative, the bound the project holds the sampler to on the same GEMM, chain length and inputs
(tests/test_gpu_sample.py: d logp <= 1e-11), and the exponent exactly wherever the mirror's mantissa is not on a power-of-two
boundary --, against ``Context.sample`` on the strings it drew, against the dense state vector on all 2^9 strings, the bit
guarantees (a state alone, the cut into chain batches, a subset and a permutation of the strings, a shared and a per-state table, two
runs, a device-built set), circuits whose outcomes are certain, a chain whose amplitudes underflow as complex128, the rejections,
and ``build_outcome_likelihoods`` against the pipeline spelled out by hand.

The inputs are those of tests/test_amplitude_host.py, which bounds the mirror's own error on them by 1e-12 (measured: 8.2e-14).

Measured on the MI355X, max |amp_hip - amp_mirror| / |amp_mirror| over the 140 strings of every state: "a12" 1.4e-13, "a9" 3.2e-13,
"two" 6.7e-16, "one" 0, "g20" 5.4e-14, "g300" 1.7e-13, the underflow case 1.2e-14 (exponents -1357 .. -1347); no exponent differs.
max |logp_hip - logp_mirror| = 2.9e-13 ("a12"); max |logp_amplitudes - logp_sample| on the device = 1.4e-14 ("g20")."""
import itertools

import numpy as np
import pytest

import qml_cutensornet_amd as Q
from helpers import SHOTS
from oracle import restatement as R
from qml_cutensornet_amd import engine
from test_amplitude_host import AMP_CASES, amp_case, amp_mirror, underflow_case
from test_sample_host import ansatz_states, dense_of_mps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device(gpu_ctx):
    """name -> (mant, expo, logp, norms) of the device for every case, one call each (per-state tables)."""
    out = {}
    for name in AMP_CASES:
        states, bits, bases = amp_case(name)
        with gpu_ctx.upload(states) as xs:
            out[name] = gpu_ctx.amplitudes(xs, bits, bases=bases, per_state=True, scaled=True, logp=True, norms=True)
    return out


def relative(mant, expo, ref_mant, ref_expo):
    """|a - a_ref| / |a_ref| of scaled amplitudes, the exponents' difference applied exactly."""
    d = np.ldexp(mant.real, expo - ref_expo) + 1j * np.ldexp(mant.imag, expo - ref_expo) - ref_mant
    return np.abs(d) / np.abs(ref_mant)


@pytest.mark.parametrize("name", AMP_CASES)
def test_device_against_the_mirror(device, name):
    """|amp_dev - amp_mirror| <= 1e-11 |amp_mirror| on the 140 strings of every state, and equal exponents off the boundaries."""
    states, bits, _ = amp_case(name)
    mant, expo, lp, _ = device[name]
    hm, he, hl = amp_mirror(name)
    ns, n = len(states), len(states[0])
    assert mant.shape == (ns, 2 * SHOTS) and mant.dtype == np.complex128 and expo.shape == (ns, 2 * SHOTS) and expo.dtype == np.int32
    if name == "a12":
        assert sorted(m.max_bond() for m in states) == [30, 41, 50, 50]
    assert np.all(np.abs(hm) > 0)
    rel = relative(mant, expo, hm, he)
    print(f"{name}: max |amp_hip - amp_mirror| / |amp_mirror| = {rel.max():.3e} over {rel.size} strings, max |d logp| = {np.abs(lp - hl).max():.3e}")
    assert rel.max() <= 1e-11
    big = np.maximum(np.abs(mant.real), np.abs(mant.imag))
    assert np.all((big >= 0.5) & (big < 1.0))
    hbig = np.maximum(np.abs(hm.real), np.abs(hm.imag))
    off = (np.abs(hbig - 0.5) > 1e-9) & (np.abs(hbig - 1.0) > 1e-9)  # a condition on the inputs: not on a power-of-two boundary
    assert off.any() and np.array_equal(expo[off], he[off])
    assert np.abs(lp - hl).max() <= 3e-11  # 2 |d amp| / |amp| and the norm's own rounding


def test_cases_cross_the_blocks(gpu_ctx):
    """From the sets' own bond tables: padded bonds of 64, 80, 128, 208 and 304, so AMP_W has up to ten column blocks and the
    64-wide loops of the pick kernel run more than once; 140 strings are two full tiles of 64 rows and a ragged one of 12."""
    for name, want in (("g20", (64, 80, 128)), ("g300", (64, 128, 208, 304))):
        with gpu_ctx.upload(amp_case(name)[0]) as xs:
            pads = set(((np.asarray(xs.dims) + 15) // 16 * 16).ravel().tolist())
        assert all(w in pads for w in want), (name, sorted(pads))
    assert 2 * SHOTS == 2 * 64 + 12


@pytest.mark.parametrize("name", ["a12", "g20", "two"])
def test_against_the_sampler(gpu_ctx, name):
    """The bits ``Context.sample`` draws, fed back with its bases: |logp_amplitudes - logp_sample| <= 3e-11, each route's 1e-11
    against its mirror plus the mirrors' own distance (tests/test_amplitude_host.py: at most 1e-12)."""
    from test_gpu_sample import cases

    states, bases, seed = cases()[name]
    with gpu_ctx.upload(states) as xs:
        bits, lp = gpu_ctx.sample(xs, SHOTS, bases=bases, seed=seed, logp=True)
        amp, la = gpu_ctx.amplitudes(xs, bits, bases=bases, per_state=True, logp=True)
    print(f"{name}: max |logp_amplitudes - logp_sample| = {np.abs(la - lp).max():.3e}")
    assert np.abs(la - lp).max() <= 3e-11
    assert amp.shape == lp.shape and amp.dtype == np.complex128


def test_dense(gpu_ctx):
    states, _ = ansatz_states(9, 2, 3, 21)
    every = np.array(list(itertools.product((0, 1), repeat=9)), dtype=np.uint8)
    with gpu_ctx.upload(states) as xs:
        amp, lp, nrm = gpu_ctx.amplitudes(xs, every, logp=True, norms=True)
    for i, m in enumerate(states):
        psi = dense_of_mps(m).reshape(-1)
        assert np.abs(amp[i] - psi).max() <= 1e-13
        assert abs(np.exp(lp[i]).sum() - 1.0) <= 1e-12
        assert abs((np.abs(amp[i]) ** 2).sum() - nrm[i]) <= 1e-12


def test_bit_guarantees(gpu_ctx, device, monkeypatch):
    states, bits, bases = amp_case("a12")
    mant, expo, lp, nrm = device["a12"]

    def same(got, rows=slice(None), cols=slice(None)):
        return all(np.array_equal(g, w[rows, cols]) for g, w in zip(got, (mant, expo, lp)))

    for i in (1, 3):  # a state alone
        with gpu_ctx.upload([states[i]]) as xs:
            assert same(gpu_ctx.amplitudes(xs, bits[i : i + 1], bases=bases, per_state=True, scaled=True, logp=True), slice(i, i + 1))
    with gpu_ctx.upload(states) as xs:
        for cap in ("1", "5"):  # 12 chains in batches of one and of five
            monkeypatch.setenv("QK_AMP_BATCH", cap)
            assert same(gpu_ctx.amplitudes(xs, bits, bases=bases, per_state=True, scaled=True, logp=True))
        monkeypatch.setenv("QK_AMP_BATCH", "0")
        with pytest.raises(engine.QkError, match="QK_AMP_BATCH"):
            gpu_ctx.amplitudes(xs, bits[0])
        monkeypatch.delenv("QK_AMP_BATCH")
        assert same(gpu_ctx.amplitudes(xs, bits, bases=bases, per_state=True, scaled=True, logp=True))  # two runs
        # a subset and a permutation of the strings: other rows of other tiles
        perm = np.random.default_rng(5).permutation(2 * SHOTS)
        for pick in (np.arange(3, 40), perm):
            assert same(gpu_ctx.amplitudes(xs, bits[:, pick], bases=bases[pick], per_state=True, scaled=True, logp=True), cols=pick)
        # a shared table against the same table repeated per state; the norms are the sweep's
        shared = gpu_ctx.amplitudes(xs, bits[2], bases=bases, scaled=True, logp=True, norms=True)
        tiled = gpu_ctx.amplitudes(xs, np.repeat(bits[2:3], len(states), axis=0), bases=bases, per_state=True, scaled=True, logp=True)
        assert all(np.array_equal(a, b) for a, b in zip(shared[:3], tiled))
        assert np.array_equal(shared[0][2], mant[2]) and np.array_equal(shared[1][2], expo[2])
        assert np.array_equal(shared[3], nrm) and np.array_equal(nrm, gpu_ctx.local_paulis(xs, norms=True)[1])
        # the default form is ldexp of the scaled one; None is all Z
        plain = gpu_ctx.amplitudes(xs, bits[2], bases=bases)
        assert isinstance(plain, np.ndarray) and np.array_equal(plain, np.ldexp(shared[0].real, shared[1]) + 1j * np.ldexp(shared[0].imag, shared[1]))
        assert np.array_equal(gpu_ctx.amplitudes(xs, bits[2]), gpu_ctx.amplitudes(xs, bits[2], bases="Z" * 12))
    # a set built on the device and its download uploaded again
    ans = Q.KernelStateAnsatz(9, 2, 1.0, Q.entanglement_graph(9, 2))
    circs = [ans.circuit_for_data(x) for x in R.synthetic_features(4, 9, 6)]
    b9, s9 = engine.random_bases(SHOTS, 9, 3), np.random.default_rng(9).integers(0, 2, (SHOTS, 9), dtype=np.uint8)
    built, _ = gpu_ctx.build_mps_set(circs)
    with built:
        tensors = built.download()
        on_device = gpu_ctx.amplitudes(built, s9, bases=b9, scaled=True, logp=True, norms=True)
    with gpu_ctx.upload(tensors) as xs:
        uploaded = gpu_ctx.amplitudes(xs, s9, bases=b9, scaled=True, logp=True, norms=True)
    assert all(np.array_equal(a, b) for a, b in zip(on_device, uploaded))


def test_exact_cases_and_underflow(gpu_ctx):
    n = 6
    zero = Q.MPS([np.array([1.0, 0.0], dtype=np.complex128).reshape(1, 2, 1) for _ in range(n)])
    strings = np.zeros((4, n), dtype=np.uint8)
    strings[1, 0] = strings[2, n - 1] = strings[3, 2] = 1
    plus = Q.simulate(Q.BoundCircuit.from_gates(1, [("H", [0], [])]), 1 - 1e-16)
    with gpu_ctx.upload([zero]) as xs:
        mant, expo, lp = gpu_ctx.amplitudes(xs, strings, scaled=True, logp=True)
    assert mant[0, 0] == 0.5 + 0j and expo[0, 0] == 1 and lp[0, 0] == 0.0
    assert np.all(mant[0, 1:] == 0) and np.all(expo[0, 1:] == 0) and np.all(lp[0, 1:] == -np.inf)
    with gpu_ctx.upload([plus]) as xs:
        a = gpu_ctx.amplitudes(xs, [[0], [1]], bases="X")
    assert abs(abs(a[0, 0]) - 1.0) <= 1e-15 and abs(a[0, 1]) <= 1e-15
    small, bits, bases = underflow_case()
    hm, he = small.amplitude(bits, bases=bases, scaled=True)
    with gpu_ctx.upload([small]) as xs:
        assert np.all(gpu_ctx.amplitudes(xs, bits, bases=bases) == 0)  # 1e-400 is no double
        mant, expo = gpu_ctx.amplitudes(xs, bits, bases=bases, scaled=True)
        with pytest.raises(engine.QkError, match="state 0"):  # <psi|psi> = 1e-800 is no double either: logp is refused, by name
            gpu_ctx.amplitudes(xs, bits, bases=bases, logp=True)
    rel = relative(mant[0], expo[0], hm, he)
    print(f"underflow case: max |amp_hip - amp_mirror| / |amp_mirror| = {rel.max():.3e}, exponents {expo.min()} .. {expo.max()}")
    assert expo.max() < -1300 and rel.max() <= 1e-11


def test_rejections(gpu_ctx):
    states, bits, bases = amp_case("a9")
    b, c = bits[0][:8], bases[:8]
    with gpu_ctx.upload(states) as xs:
        with xs.to_f32() as x32:
            with pytest.raises(engine.QkError, match="set is complex64"):
                gpu_ctx.amplitudes(x32, b)
        with pytest.raises(engine.QkError, match="n_strings"):
            gpu_ctx.amplitudes(xs, b[:0])
        bad = b.copy()
        bad[5, 3] = 2
        with pytest.raises(engine.QkError, match=r"bits\[5\]\[3\] = 2"):
            gpu_ctx.amplitudes(xs, bad, bases=c)
        bad3 = np.repeat(b[None], len(states), axis=0)
        bad3[1, 4, 2] = 7
        with pytest.raises(engine.QkError, match=r"bits\[1\]\[4\]\[2\] = 7"):
            gpu_ctx.amplitudes(xs, bad3, per_state=True)
        for code in (0, 4):
            badc = c.copy()
            badc[5, 3] = code
            with pytest.raises(engine.QkError, match=rf"bases\[5\]\[3\] = {code}"):
                gpu_ctx.amplitudes(xs, b, bases=badc)
        for wrong in (b[:, :8], b[0], np.ones((8, 9)), np.repeat(b[None], 2, axis=0)):
            with pytest.raises(ValueError, match="bits"):
                gpu_ctx.amplitudes(xs, wrong, per_state=np.ndim(wrong) == 3)
        with pytest.raises(ValueError, match="bases"):
            gpu_ctx.amplitudes(xs, b, bases=c[:7])
        # the C entry point itself names what it rejects
        L, h = engine.lib(), gpu_ctx.handle
        mant, expo = np.zeros((len(states), 8, 2)), np.zeros((len(states), 8), dtype=np.int32)
        args = dict(ctx=h, set=xs.handle, n=8, bits=b.ctypes.data, per=0, bases=None, mant=mant.ctypes.data, expo=expo.ctypes.data)
        for change, word in ((dict(ctx=None), "ctx"), (dict(set=None), "set"), (dict(bits=None), "bits"), (dict(mant=None), "mant"), (dict(expo=None), "expo"),
                             (dict(per=2), "bits_per_state"), (dict(per=-1), "bits_per_state")):
            a = {**args, **change}
            rc = L.qk_amplitudes_host(a["ctx"], a["set"], a["n"], a["bits"], a["per"], a["bases"], a["mant"], a["expo"], None, None)
            assert rc != 0 and word in L.qk_last_error().decode(), (word, L.qk_last_error())
        with engine.Context(0) as other:
            with pytest.raises(engine.QkError, match="another context"):
                other.amplitudes(xs, b)
        # a state of norm 0 is named when logp is asked for, and is no error otherwise
        zero = Q.MPS([0.0 * t for t in states[1].tensors])
    with gpu_ctx.upload([states[0], zero]) as xs:
        with pytest.raises(engine.QkError, match="state 1"):
            gpu_ctx.amplitudes(xs, b, logp=True)
        mant, expo = gpu_ctx.amplitudes(xs, b, scaled=True)
        assert np.all(mant[1] == 0) and np.all(expo[1] == 0) and np.all(mant[0] != 0)


E2E = dict(n=10, layers=2, nx=9, strings=64)


def test_build_outcome_likelihoods(gpu_ctx, monkeypatch):
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import _simulate_share, build_outcome_likelihoods

    monkeypatch.setenv("QK_BUILDER", "host")
    n, S = E2E["n"], E2E["strings"]
    ans = Q.KernelStateAnsatz(n, E2E["layers"], 1.0, Q.entanglement_graph(n, 2))
    X = R.synthetic_features(E2E["nx"], n, 13)
    bases = engine.random_bases(S, n, 21)
    ctx = engine.default_context(0)
    _, xs, _, _ = _simulate_share(ans, np.asarray(X, dtype=np.float64), 0, 1, 1 - 1e-16, False, "X")
    shots = ctx.sample(xs, S, bases=bases, seed=3)  # the "hardware" shots of every state
    hand_own = ctx.amplitudes(xs, shots, bases=bases, per_state=True, logp=True)[1]
    hand_cross = ctx.amplitudes(xs, shots[4], bases=bases, logp=True)[1]
    xs.close()
    own = build_outcome_likelihoods(SingleComm(), ans, X, shots, bases=bases, per_state=True, truncation_error=1e-16)
    cross = build_outcome_likelihoods(SingleComm(), ans, X, shots[4], bases=bases, truncation_error=1e-16)
    assert own.shape == (E2E["nx"], S) and np.array_equal(own, hand_own)
    assert cross.shape == (E2E["nx"], S) and np.array_equal(cross, hand_cross) and np.array_equal(cross[4], own[4])
    # maximum likelihood finds the state the shots came from, and its own shots score a positive log XEB
    assert int(np.argmax(cross.sum(axis=1))) == 4
    assert np.all(engine.xeb_fidelity(own, n, kind="log") > 0)
    with pytest.raises(ValueError, match="bits"):
        build_outcome_likelihoods(SingleComm(), ans, X, shots, bases=bases, truncation_error=1e-16)
    with pytest.raises(ValueError, match="truncation"):
        build_outcome_likelihoods(SingleComm(), ans, X, shots[4])
