"""Windows of k qubits on the MI355X: qk_window_rdms_host against a plain einsum reference from ``helpers.environments`` on
general-gauge states (dense complex L_k and R_k, bonds across the 16-row padding and the 64-wide blocks, bond 300), against dense
state vectors for widths 5 and 6, the edge chains, the identities with the sibling sweeps, the bit guarantees (a state alone, a
subset of the starts, QK_WINDOW_BATCH, two runs, the norms), the rejections, and build_projected_kernel_matrix(rdm=3,
window=True) with one and two ranks.  The tolerances are the siblings' on the same inputs; a comparison asserts that at least half
of the off-diagonal reference entries are >= 1e-3 in magnitude in the real and in the imaginary part, so that a wrong conjugate or plane cannot hide
behind zeros."""
import os
import sys

import numpy as np
import pytest

import qml_cutensornet_amd as Q
from helpers import environments, gauge_set_300, gauge_sets, scrambled
from oracle import restatement as R
from qml_cutensornet_amd import engine
from test_projected_host import dense

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ref_window(tensors, env, a, w):
    """rho_{a,w} by one einsum over L_a, the product of the window's sites and R_b."""
    L, Rr = env
    ts = [np.asarray(t, dtype=np.complex128) for t in tensors]
    M = ts[a]
    for k in range(a + 1, a + w):
        M = np.tensordot(M, ts[k], axes=(2, 0)).reshape(M.shape[0], -1, ts[k].shape[2])
    rho = np.einsum("ab,asc,cd,btd->st", L[a], M, Rr[a + w], M.conj(), optimize=True)
    return rho / L[len(ts)][0, 0].real


def ref_windows(states, w, starts=None):
    out = []
    for m in states:
        env = environments(m.tensors)
        st = range(len(m) - w + 1) if starts is None else starts
        out.append(np.stack([ref_window(m.tensors, env, a, w) for a in st]))
    return np.stack(out)


def dense_windows(states, w, starts=None):
    out = []
    for m in states:
        psi, n = dense(m), len(m)
        st = range(n - w + 1) if starts is None else starts
        rows = []
        for a in st:
            t = psi.reshape(2**a, 2**w, -1)
            rows.append(np.einsum("lsr,ltr->st", t, t.conj()) / float(np.vdot(psi, psi).real))
        out.append(np.stack(rows))
    return np.stack(out)


def offdiag_shares(ref):
    D = ref.shape[-1]
    off = ref[..., ~np.eye(D, dtype=bool)]
    return float((np.abs(off.real) >= 1e-3).mean()), float((np.abs(off.imag) >= 1e-3).mean())


def check_structure(rho, label=""):
    """Exactly Hermitian, a zero imaginary diagonal, trace 1."""
    assert rho.dtype == np.complex128
    assert np.array_equal(rho, rho.conj().swapaxes(-1, -2))
    d = np.arange(rho.shape[-1])
    assert np.all(rho[..., d, d].imag == 0.0)
    tr = float(np.abs(np.trace(rho, axis1=-2, axis2=-1) - 1.0).max())
    print(f"{label}: max |tr rho - 1| = {tr:.3e}")
    assert tr < 1e-13


def check_against(rho, ref, tol, label, shares=True):
    err = float(np.abs(rho - ref).max())
    sr, si = offdiag_shares(ref)
    print(f"{label}: rho {rho.shape}, max |d rho| = {err:.3e}, off-diagonal shares >= 1e-3: Re {sr:.2f}, Im {si:.2f}")
    if shares:
        assert sr >= 0.5 and si >= 0.5
    assert err < tol


# ---- 1. general-gauge sets against the einsum reference --------------------------------------------------------------------
@pytest.fixture(scope="module")
def gauge_dev(gpu_ctx):
    originals, twins = gauge_sets()
    with gpu_ctx.upload(list(twins)) as dt, gpu_ctx.upload(list(originals)) as do:
        yield dt, do


@pytest.fixture(scope="module")
def gauge_rdms(gpu_ctx, gauge_dev):
    """The device RDMs of the six twins, every window, widths 1 .. 4: computed once, shared and left unchanged."""
    dt, _ = gauge_dev
    out = {w: gpu_ctx.window_rdms(dt, w) for w in range(1, 5)}
    for r in out.values():
        r.setflags(write=False)
    return out


@pytest.mark.parametrize("w", [1, 2, 3, 4])
def test_gauge_twins_against_einsum(gpu_ctx, gauge_dev, gauge_rdms, w):
    originals, twins = gauge_sets()
    _, do = gauge_dev
    rho = gauge_rdms[w]
    assert rho.shape == (6, 20 - w + 1, 2**w, 2**w)
    check_structure(rho, f"twins, w = {w}")
    check_against(rho, ref_windows(twins, w), 1e-12, f"twins vs einsum, w = {w}")
    ro = gpu_ctx.window_rdms(do, w)
    check_structure(ro, f"originals, w = {w}")
    err = float(np.abs(rho - ro).max())
    print(f"twins vs originals on the device, w = {w}: max |d rho| = {err:.3e}")
    assert err < 1e-12


# ---- 2. widths 5 and 6 against dense state vectors -----------------------------------------------------------------------------
def wide_chains():
    rng = np.random.default_rng(612)
    out = []
    for k in range(3):
        m = Q.random_mps(12, [1, 2, 4, 8, 16, 17, 20, 17, 16, 8, 4, 2, 1], rng)
        out.append(scrambled(m, rng, scale=3.7 if k % 2 else 1.0))
    return out


@pytest.mark.parametrize("w", [5, 6])
def test_wide_windows_against_dense(gpu_ctx, w):
    states = wide_chains()
    with gpu_ctx.upload(states) as xs:
        rho = gpu_ctx.window_rdms(xs, w)
        ends = gpu_ctx.window_rdms(xs, w, starts=(0, 12 - w))
    check_structure(rho, f"12 sites, w = {w}")
    check_against(rho, dense_windows(states, w), 1e-12, f"12 sites vs dense, w = {w}")
    check_against(ends, dense_windows(states, w, (0, 12 - w)), 1e-12, f"12 sites vs dense, both ends, w = {w}")
    assert np.array_equal(ends, rho[:, [0, 12 - w]])


# ---- 3. bond 300 ----------------------------------------------------------------------------------------------------------------
def test_bond_300(gpu_ctx):
    _, twins = gauge_set_300()
    starts = (7, 8, 9)
    with gpu_ctx.upload(list(twins)) as xs:
        rho = gpu_ctx.window_rdms(xs, 2, starts=starts)
    check_structure(rho, "bond 300")
    check_against(rho, ref_windows(twins, 2, starts), 1e-12, "bond 300 vs einsum, w = 2")


# ---- 4. edge chains -------------------------------------------------------------------------------------------------------------
def test_edge_chains(gpu_ctx):
    rng = np.random.default_rng(4)
    one = [Q.MPS([(rng.standard_normal((1, 2, 1)) + 1j * rng.standard_normal((1, 2, 1))) * f]) for f in (1.0, 2.5)]
    with gpu_ctx.upload(one) as xs:
        rho = gpu_ctx.window_rdms(xs, 1)
    check_structure(rho, "n = 1")
    check_against(rho, dense_windows(one, 1), 1e-12, "n = 1, w = 1", shares=False)
    two = [scrambled(Q.random_mps(2, [1, 2, 1], rng), rng, scale=s) for s in (1.0, 3.7)]
    with gpu_ctx.upload(two) as xs:
        for w in (1, 2):
            rho = gpu_ctx.window_rdms(xs, w)
            assert rho.shape == (2, 3 - w, 2**w, 2**w)
            check_structure(rho, f"n = 2, w = {w}")
            check_against(rho, dense_windows(two, w), 1e-12, f"n = 2, w = {w}", shares=False)
    six = [scrambled(Q.random_mps(6, [1, 2, 4, 8, 4, 2, 1], rng), rng, scale=s) for s in (1.0, 3.7, 0.4)]
    with gpu_ctx.upload(six) as xs:
        rho, norms = gpu_ctx.window_rdms(xs, 6, norms=True)
        fid = gpu_ctx.gram(xs)
    assert rho.shape == (3, 1, 64, 64)
    check_structure(rho, "w = n = 6")
    check_against(rho, dense_windows(six, 6), 1e-12, "w = n = 6")
    O, Sx, _ = engine.window_overlaps(rho)
    err = float(np.abs(O[0] - fid / np.outer(norms, norms)).max())
    print(f"w = n = 6: max |O - gram / norms| = {err:.3e}, max |S - 1| = {float(np.abs(Sx - 1).max()):.3e}")
    assert err < 1e-12 and np.abs(Sx - 1.0).max() < 1e-12


# ---- 5. identities against the siblings on the device ------------------------------------------------------------------------
def test_identities_with_the_siblings(gpu_ctx, gauge_dev, gauge_rdms):
    dt, _ = gauge_dev
    n = 20
    F = gpu_ctx.local_paulis(dt)
    c1 = engine.rdm_paulis(gauge_rdms[1])
    e1 = float(np.abs(c1[..., 1:] - F).max())
    T = gpu_ctx.local_pair_paulis(dt)
    c2 = engine.rdm_paulis(gauge_rdms[2])
    e2 = float(np.abs(c2 - T).max())
    print(f"w = 1 vs local_paulis: {e1:.3e}; w = 2 vs local_pair_paulis: {e2:.3e}")
    assert e1 < 1e-12 and np.abs(c1[..., 0] - 1.0).max() < 1e-12 and e2 < 1e-12
    # Pauli coefficients of three-qubit windows against pauli_expectations of the same strings
    rng = np.random.default_rng(5)
    c3 = engine.rdm_paulis(gauge_rdms[3])
    picks = [(int(a), tuple(int(v) for v in rng.integers(0, 4, 3))) for a in rng.integers(0, n - 2, 40)]
    picks = [(a, p) for a, p in picks if any(p)]
    S = np.zeros((len(picks), n), dtype=np.uint8)
    for r, (a, p) in enumerate(picks):
        S[r, a : a + 3] = p
    V = gpu_ctx.pauli_expectations(dt, S)
    got = np.stack([c3[(slice(None), a) + p] for a, p in picks], axis=1)
    e3 = float(np.abs(got - V).max())
    print(f"rdm_paulis of w = 3 vs pauli_expectations ({len(picks)} strings): {e3:.3e}, share of |V| >= 1e-3: {float((np.abs(V) >= 1e-3).mean()):.2f}")
    assert e3 < 1e-12
    pur = gpu_ctx.bond_purities(dt)
    for w in range(1, 5):
        O, Sx, _ = engine.window_overlaps(gauge_rdms[w])
        assert np.array_equal(O, O.transpose(0, 2, 1)) and np.array_equal(O[:, np.arange(6), np.arange(6)], Sx)
        ep = max(float(np.abs(Sx[0] - pur[:, w - 1]).max()), float(np.abs(Sx[n - w] - pur[:, n - w - 1]).max()))
        Ol = gpu_ctx.block_overlaps(dt, None, [w], "left")[0][0]
        Or = gpu_ctx.block_overlaps(dt, None, [w], "right")[0][0]
        eo = max(float(np.abs(O[0] - Ol).max()), float(np.abs(O[n - w] - Or).max()))
        print(f"w = {w}: purities at the ends vs bond_purities {ep:.3e}, overlaps at the ends vs block_overlaps {eo:.3e}")
        assert ep < 1e-12 and eo < 1e-12
        K = engine.block_kernel(O[3], Sx[3], form="normalized")
        assert np.array_equal(K, K.T) and np.all(np.diag(K) == 1.0)


def test_projected_window_gram(gpu_ctx, gauge_dev, gauge_rdms):
    dt, _ = gauge_dev
    g = 0.37
    K1 = gpu_ctx.projected_window_gram(gauge_rdms[1], gamma=g)
    K2 = gpu_ctx.projected_window_gram(gauge_rdms[2], gamma=g)
    e1 = float(np.abs(K1 - gpu_ctx.projected_gram(gpu_ctx.local_paulis(dt), gamma=g)).max())
    e2 = float(np.abs(K2 - gpu_ctx.projected_pair_gram(gpu_ctx.local_pair_paulis(dt), gamma=g)).max())
    print(f"projected_window_gram vs projected_gram (w = 1): {e1:.3e}, vs projected_pair_gram (w = 2): {e2:.3e}")
    assert e1 < 1e-13 and e2 < 1e-13
    for w in (1, 2, 3):
        r = gauge_rdms[w]
        d = r[None, :] - r[:, None]
        ref = np.exp(-g * (np.abs(d) ** 2).sum(axis=(2, 3, 4)))
        K = gpu_ctx.projected_window_gram(r, gamma=g)
        err = float(np.abs(K - ref).max())
        print(f"projected_window_gram vs numpy, w = {w}: {err:.3e}, median off-diagonal {float(np.median(K[~np.eye(6, dtype=bool)])):.3f}")
        assert err < 1e-13 and np.array_equal(K, K.T) and np.all(np.diag(K) == 1.0)
        Kt = gpu_ctx.projected_window_gram(r[:4], r[2:], gamma=g)
        assert Kt.shape == (4, 4) and np.abs(Kt - ref[2:, :4]).max() < 1e-13
    # the default bandwidth: 1 / (n_windows + width - 1) = 1 / n_sites when every window was taken
    assert np.array_equal(gpu_ctx.projected_window_gram(gauge_rdms[3]), gpu_ctx.projected_window_gram(gauge_rdms[3], gamma=1.0 / 20))


# ---- 6. bits ---------------------------------------------------------------------------------------------------------------------
def test_bits(gpu_ctx, gauge_dev, gauge_rdms, monkeypatch):
    _, twins = gauge_sets()
    dt, _ = gauge_dev
    w = 3
    full = gauge_rdms[w]
    rho, norms = gpu_ctx.window_rdms(dt, w, norms=True)  # a second run
    assert np.array_equal(rho, full)
    assert np.array_equal(norms, gpu_ctx.local_paulis(dt, norms=True)[1])
    with gpu_ctx.upload([twins[3]]) as alone:
        assert np.array_equal(gpu_ctx.window_rdms(alone, w)[0], full[3])
    sub = (0, 5, 6, 12, 17)
    assert np.array_equal(gpu_ctx.window_rdms(dt, w, starts=sub), full[:, list(sub)])
    for cap in ("1", "3"):
        monkeypatch.setenv("QK_WINDOW_BATCH", cap)
        assert np.array_equal(gpu_ctx.window_rdms(dt, w, starts=sub), full[:, list(sub)])
        assert np.array_equal(gpu_ctx.window_rdms(dt, 1), gauge_rdms[1])
    monkeypatch.setenv("QK_WINDOW_BATCH", "0")
    with pytest.raises(engine.QkError, match="QK_WINDOW_BATCH"):
        gpu_ctx.window_rdms(dt, 1)


# ---- 7. rejections ---------------------------------------------------------------------------------------------------------------
def test_rejections(gpu_ctx, gauge_dev):
    dt, _ = gauge_dev
    L = engine.lib()
    rho = np.zeros((6, 20, 2, 2), dtype=np.complex128)
    st = np.array([0, 1], dtype=np.int32)

    def raw(*args):
        engine._check(L.qk_window_rdms_host(*args), "qk_window_rdms_host")

    for args, name in (((None, dt.handle, 1, 0, None, rho.ctypes.data, None), "ctx"), ((gpu_ctx.handle, None, 1, 0, None, rho.ctypes.data, None), "set"),
                       ((gpu_ctx.handle, dt.handle, 1, 0, None, None, None), "rho")):
        with pytest.raises(engine.QkError, match=f"{name} is null"):
            raw(*args)
    other = engine.Context(0)
    try:
        with other.upload([gauge_sets()[1][2]]) as os_:
            with pytest.raises(engine.QkError, match="another context"):
                gpu_ctx.window_rdms(os_, 1)
    finally:
        other.close()
    with dt.to_f32() as f32:
        with pytest.raises(engine.QkError, match="complex64"):
            gpu_ctx.window_rdms(f32, 1)
    for w in (0, 7, -1):
        with pytest.raises(engine.QkError, match="width"):
            gpu_ctx.window_rdms(dt, w)
    with gpu_ctx.upload([Q.random_mps(4, [1, 2, 4, 2, 1], np.random.default_rng(0))]) as short:
        with pytest.raises(engine.QkError, match="width"):
            gpu_ctx.window_rdms(short, 5)
    for bad in ((-1, 2), (0, 19), (3, 3), (5, 4)):  # outside 0 .. n - w = 18 (w = 2), or not strictly increasing
        with pytest.raises(engine.QkError, match="starts"):
            gpu_ctx.window_rdms(dt, 2, starts=bad)
    with pytest.raises(engine.QkError, match="n_starts"):
        gpu_ctx.window_rdms(dt, 2, starts=())
    with pytest.raises(engine.QkError, match="n_starts"):
        raw(gpu_ctx.handle, dt.handle, 1, -2, st.ctypes.data, rho.ctypes.data, None)
    zero = [Q.random_mps(4, [1, 2, 4, 2, 1], np.random.default_rng(1)),
            Q.MPS([np.zeros((l, 2, r), dtype=np.complex128) for l, r in ((1, 2), (2, 4), (4, 2), (2, 1))])]
    with gpu_ctx.upload(zero) as zs:
        with pytest.raises(engine.QkError, match="state 1 has norm 0"):
            gpu_ctx.window_rdms(zs, 2)
    with pytest.raises(ValueError, match="width"):
        gpu_ctx.window_rdms(dt, 2.0)
    with pytest.raises(ValueError, match="starts"):
        gpu_ctx.window_rdms(dt, 2, starts=[0.5])


# ---- 8. build_projected_kernel_matrix(rdm=3, window=True) ----------------------------------------------------------------------
def _exact_windows(ans, x, w):
    circ = ans.circuit_for_data(x)
    n = circ.n_qubits
    psi = R.statevector(n, [(name, tuple(qs), (p[0] if p else None)) for name, qs, p in circ.as_tuples()])
    rows = []
    for a in range(n - w + 1):
        t = np.asarray(psi).reshape(2**a, 2**w, -1)
        rows.append(np.einsum("lsr,ltr->st", t, t.conj()) / float(np.vdot(psi, psi).real))
    return np.stack(rows)


def _exact_kernel(ans, X, Y, g, w):
    rx = np.stack([_exact_windows(ans, x, w) for x in X])
    ry = rx if Y is None else np.stack([_exact_windows(ans, y, w) for y in Y])
    d = rx[None, :] - ry[:, None]
    return np.exp(-g * (np.abs(d) ** 2).sum(axis=(2, 3, 4)))


def _case():
    n = 10
    return Q.KernelStateAnsatz(n, 2, 1.0, Q.entanglement_graph(n, 2)), R.synthetic_features(7, n, 21), R.synthetic_features(4, n, 22)


def test_build_projected_kernel_matrix_window_exact(gpu_ctx, tmp_path):
    import json

    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_projected_kernel_matrix

    ans, X, Y = _case()
    info = str(tmp_path / "prof")
    K = build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, info_file=info, rdm=3, window=True)
    err = float(np.abs(K - _exact_kernel(ans, X, None, 1.0 / 10, 3)).max())
    Kt = build_projected_kernel_matrix(SingleComm(), ans, X, Y=Y, pqk_gamma=0.2, truncation_error=1e-16, rdm=3, window=True)
    err_t = float(np.abs(Kt - _exact_kernel(ans, X, Y, 0.2, 3)).max())
    print(f"build_projected_kernel_matrix(rdm=3, window=True): train max |dK| = {err:.3e}, test max |dK| = {err_t:.3e}")
    assert K.shape == (7, 7) and Kt.shape == (4, 7) and err < 1e-10 and err_t < 1e-10
    prof = json.load(open(info + ".json"))
    assert prof["pqk_rdm"] == [3, "qubits"] and prof["pqk_gamma"][0] == 1.0 / 10 and "pqk_pair_distance" not in prof
    for kw in (dict(rdm=3, pair_distance=2), dict(rdm=3, shots=10), dict(rdm=3, observables=["ZZ"]), dict(rdm=7), dict(rdm=11), dict(rdm=2),
               dict(rdm=1)):
        with pytest.raises(ValueError):
            build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, window=True, **kw)
    with pytest.raises(ValueError, match="window=True"):  # rdm >= 3 alone stays the error it was before the window form
        build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, rdm=3)


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["QK_BUILDER"] = "host"
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from qml_cutensornet_amd.dist import TorchComm
        from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_projected_kernel_matrix
        from test_gpu_window import _case as case_

        ans, X, Y = case_()
        comm = TorchComm()
        out = {"train": build_projected_kernel_matrix(comm, ans, X, truncation_error=1e-16, rdm=3, window=True),
               "test": build_projected_kernel_matrix(comm, ans, X, Y=Y, truncation_error=1e-16, rdm=3, window=True)}
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
    port = 29600 + ((os.getpid() + 1313) % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert res[1]["train"] is None and res[1]["test"] is None
    monkeypatch.setenv("QK_BUILDER", "host")
    ans, X, Y = _case()
    one = build_projected_kernel_matrix(SingleComm(), ans, X, truncation_error=1e-16, rdm=3, window=True)
    one_t = build_projected_kernel_matrix(SingleComm(), ans, X, Y=Y, truncation_error=1e-16, rdm=3, window=True)
    assert np.array_equal(res[0]["train"], one)
    assert np.array_equal(res[0]["test"], one_t)
