"""Amplitudes of given strings on the host (no GPU): the numpy mirror ``MPS.amplitude`` -- the loop of qk_amplitudes_host, power-of-
two rescale included -- against dense state vectors, circuits whose outcomes are certain, a chain whose amplitudes underflow as
complex128, the conditioning of the inputs of tests/test_gpu_amplitude.py (the float64 loop against the same loop in extended
precision, so that the GPU tolerance is a statement about the device), ``logp`` against the sampler's mirror on the strings it drew,
and ``engine.xeb_fidelity`` on a table made by hand.

Measured on the CPU (max relative |amp_f64 - amp_longdouble|, the 70 drawn and the 70 random strings of every state): "a12" 7.3e-14,
"a9" 8.2e-14, "two" 5.9e-16, "g20" 4.5e-14, "g300" (first 8 of each kind) 1.3e-14, the underflow case 6.7e-15; max
|logp_amplitude - logp_sample| = 2.3e-14 ("g20")."""
import functools
import itertools

import numpy as np
import pytest

import qml_cutensornet_amd as Q
from helpers import SHOTS
from qml_cutensornet_amd import engine
from test_sample_host import OUTCOME_ROWS, ansatz_states, dense_of_mps, dense_probability

AMP_CASES = ["a12", "a9", "two", "one", "g20", "g300"]


@functools.lru_cache(maxsize=None)
def amp_case(name):
    """(states, bits (n_states, 2 SHOTS, n), bases (2 SHOTS, n)) of a case of tests/test_gpu_sample.py: per state the SHOTS strings
    its mirror sampler draws in the case's bases and, in the same bases again, SHOTS uniform random strings (default_rng(1000 + i))."""
    from test_gpu_sample import cases, mirror

    states, bases, _ = cases()[name]
    drawn = mirror(name)[0]
    n = len(states[0])
    rand = np.stack([np.random.default_rng(1000 + i).integers(0, 2, (SHOTS, n), dtype=np.uint8) for i in range(len(states))])
    return states, np.concatenate([drawn, rand], axis=1), np.concatenate([bases, bases], axis=0)


@functools.lru_cache(maxsize=None)
def amp_mirror(name):
    """(mant (n_states, 2 SHOTS) complex128, expo int32, logp) of the host mirror for every state of a case."""
    states, bits, bases = amp_case(name)
    out = [m.amplitude(bits[i], bases=bases, scaled=True, logp=True) for i, m in enumerate(states)]
    return tuple(np.stack([o[j] for o in out]) for j in range(3))


def underflow_case():
    """A 40-site chi = 4 random_mps with every tensor multiplied by 1e-10 (amplitudes near 1e-406), 24 strings in random bases."""
    rng = np.random.default_rng(40)
    m = Q.random_mps(40, [1, 2] + [4] * 37 + [2, 1], rng)
    small = Q.MPS([1e-10 * np.asarray(t) for t in m.tensors])
    return small, rng.integers(0, 2, (24, 40), dtype=np.uint8), engine.random_bases(24, 40, 5)


def dense_amplitude(psi, bits, bases):
    """<b| U_bases |psi> of every string: bits and bases (strings, n), psi (2,) * n."""
    out = np.zeros(len(bits), dtype=complex)
    for s, (b, c) in enumerate(zip(bits, bases)):
        amp = psi
        for k in range(psi.ndim):
            amp = np.tensordot(OUTCOME_ROWS[int(c[k])][int(b[k])], amp, axes=(0, 0))
        out[s] = complex(amp)
    return out


def as_longdouble(mant, expo):
    return np.ldexp(np.asarray(mant.real, dtype=np.longdouble), expo) + 1j * np.ldexp(np.asarray(mant.imag, dtype=np.longdouble), expo)


def test_mirror_against_the_dense_vector():
    states, _ = ansatz_states(9, 2, 3, 21)
    every = np.array(list(itertools.product((0, 1), repeat=9)), dtype=np.uint8)
    rng = np.random.default_rng(3)
    some, bases = rng.integers(0, 2, (70, 9), dtype=np.uint8), engine.random_bases(70, 9, 3)
    for m in states:
        psi = dense_of_mps(m)
        amp = m.amplitude(every)
        assert amp.shape == (512,) and amp.dtype == np.complex128
        assert np.abs(amp - psi.reshape(-1)).max() <= 1e-14
        assert abs((np.abs(amp) ** 2).sum() - np.vdot(psi, psi).real) <= 1e-13
        mant, expo = m.amplitude(every, scaled=True)
        big = np.maximum(np.abs(mant.real), np.abs(mant.imag))
        assert expo.dtype == np.int32 and np.all((big >= 0.5) & (big < 1.0))
        assert np.array_equal(np.ldexp(mant.real, expo) + 1j * np.ldexp(mant.imag, expo), amp)
        # random bases: |amplitude|^2 / <psi|psi> is the Born probability of the string in those bases
        a, lp = m.amplitude(some, bases=bases, logp=True)
        exact = dense_probability(psi, some, bases)
        assert np.abs(a - dense_amplitude(psi, some, bases)).max() <= 1e-14
        assert np.abs(np.abs(a) ** 2 / np.vdot(psi, psi).real - exact).max() <= 1e-14
        assert np.abs(np.exp(lp) - exact).max() <= 1e-13
        # a single string is a scalar, and a row of a table
        assert m.amplitude(some[5], bases=bases[5]) == a[5] and np.shape(m.amplitude(some[5], bases=bases[5])) == ()
    # the norm is seen: 3 psi has 3 times the amplitude and the same logp
    m = states[0]
    m3 = Q.MPS([t * (3.0 if k == 0 else 1.0) for k, t in enumerate(m.tensors)])
    a, lp = m.amplitude(some, bases=bases, logp=True)
    a3, lp3 = m3.amplitude(some, bases=bases, logp=True)
    assert np.abs(a3 - 3.0 * a).max() <= 1e-14 and np.abs(lp3 - lp).max() <= 1e-13


def test_certain_outcomes():
    n = 6
    zero = Q.MPS([np.array([1.0, 0.0], dtype=np.complex128).reshape(1, 2, 1) for _ in range(n)])
    strings = np.zeros((4, n), dtype=np.uint8)
    strings[1, 0] = strings[2, n - 1] = strings[3, 2] = 1
    mant, expo, lp = zero.amplitude(strings, scaled=True, logp=True)
    assert mant[0] == 0.5 + 0j and expo[0] == 1 and lp[0] == 0.0
    assert np.all(mant[1:] == 0) and np.all(expo[1:] == 0) and np.all(lp[1:] == -np.inf)
    assert np.array_equal(zero.amplitude(strings), [1, 0, 0, 0])
    # H|0> in X: outcome 1 (eigenvalue -1) never happens
    plus = Q.simulate(Q.BoundCircuit.from_gates(1, [("H", [0], [])]), 1 - 1e-16)
    a = plus.amplitude([[0], [1]], bases="X")
    assert abs(abs(a[0]) - 1.0) <= 1e-15 and abs(a[1]) <= 1e-15
    assert np.abs(np.abs(plus.amplitude([[0], [1]])) - 0.70710678118654752440).max() <= 1e-15
    with pytest.raises(ValueError, match="bits"):
        plus.amplitude([[2]])
    with pytest.raises(ValueError, match="bits"):
        plus.amplitude([[0, 1]])
    with pytest.raises(ValueError, match="bases"):
        plus.amplitude([[0]], bases=[4])
    with pytest.raises(ValueError, match="norm 0"):
        Q.MPS([0.0 * t for t in plus.tensors]).amplitude([[0]], logp=True)


def test_underflow_survives_in_the_scaled_form():
    small, bits, bases = underflow_case()
    assert np.all(small.amplitude(bits, bases=bases) == 0)  # 1e-400: below the smallest double
    mant, expo = small.amplitude(bits, bases=bases, scaled=True)
    big = np.maximum(np.abs(mant.real), np.abs(mant.imag))
    assert np.all((big >= 0.5) & (big < 1.0)) and expo.max() < -1300
    lm, le = small.amplitude(bits, bases=bases, scaled=True, dtype=np.clongdouble)
    # mantissas in extended precision, the exponents' difference applied exactly
    d = np.ldexp(np.asarray(mant.real, dtype=np.longdouble), expo - le) + 1j * np.ldexp(np.asarray(mant.imag, dtype=np.longdouble), expo - le) - lm
    rel = float((np.abs(d) / np.abs(lm)).max())
    print(f"underflow case: max relative |amp_f64 - amp_longdouble| = {rel:.3e}")
    assert rel <= 1e-13


@pytest.mark.parametrize("name", ["a12", "a9", "two", "g20", "g300"])
def test_gpu_inputs_are_well_conditioned(name):
    """The float64 mirror is within 1e-12 relative of the same loop in extended precision on the strings of the GPU test."""
    states, bits, bases = amp_case(name)
    mant, expo, _ = amp_mirror(name)
    pick = np.r_[0:8, SHOTS : SHOTS + 8] if name == "g300" else np.arange(2 * SHOTS)  # the long-double loop takes minutes on all of "g300"
    worst = 0.0
    for i, m in enumerate(states):
        ref = m.amplitude(bits[i][pick], bases=bases[pick], dtype=np.clongdouble)
        got = as_longdouble(mant[i][pick], expo[i][pick])
        assert np.all(np.abs(ref) > 0)
        worst = max(worst, float((np.abs(got - ref) / np.abs(ref)).max()))
    print(f"{name}: max relative |amp_f64 - amp_longdouble| = {worst:.3e} over {len(states) * len(pick)} strings")
    assert worst <= 1e-12


@pytest.mark.parametrize("name", ["a12", "a9", "two", "one", "g20", "g300"])
def test_logp_against_the_sampler_mirror(name):
    from test_gpu_sample import mirror

    lp = amp_mirror(name)[2][:, :SHOTS]
    worst = float(np.abs(lp - mirror(name)[1]).max())
    print(f"{name}: max |logp_amplitude - logp_sample| = {worst:.3e}")
    assert worst <= 1e-12


def test_xeb_fidelity_by_hand():
    n = 3
    p = np.array([[1 / 8, 1 / 8, 1 / 8, 1 / 8], [1 / 4, 1 / 8, 1 / 2, 1 / 8], [1.0, 1.0, 1.0, 1.0]])
    lin = engine.xeb_fidelity(np.log(p), n)
    assert lin.shape == (3,) and np.abs(lin - [0.0, 1.0, 7.0]).max() <= 1e-14
    log = engine.xeb_fidelity(np.log(p), n, kind="log")
    want = n * np.log(2.0) + 0.57721566490153286 + np.log(p).mean(axis=1)
    assert np.abs(log - want).max() <= 1e-14 and abs(log[0] - 0.57721566490153286) <= 1e-14
    assert engine.xeb_fidelity(np.log(p[1]), n).shape == ()
    # a string of probability 0: the linear form counts it as 0, the log form is -inf
    lp0 = np.array([-np.inf, np.log(0.25)])
    assert abs(engine.xeb_fidelity(lp0, 2) - (4 * 0.125 - 1)) <= 1e-15 and engine.xeb_fidelity(lp0, 2, kind="log") == -np.inf
    with pytest.raises(ValueError, match="kind"):
        engine.xeb_fidelity(np.log(p), n, kind="xeb")
    with pytest.raises(ValueError, match="logp"):
        engine.xeb_fidelity(np.zeros((2, 0)), n)


def test_symbol_is_declared():
    assert "qk_amplitudes_host" in engine.EXPORTED_SYMBOLS
