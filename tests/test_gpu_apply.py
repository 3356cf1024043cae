"""Applying an MPO to a device-resident set on the MI355X: qk_mps_set_apply_mpo (``Context.apply_mpo``) against the numpy mirror
``MPS.apply_mpo``, element by element over the whole padded image; the bit guarantees; the consumers of the product (overlaps,
``operator_matrix``, ``compress``, the seeded builder); the driver ``build_symmetrized_kernel_matrix`` against dense state vectors
and on two ranks; every rejection.

The element bound is the issue's: |dev - mirror| <= 8 * 2^-53 * sum_s (|Re W| + |Im W|)(|Re A| + |Im A|) -- the device and the
mirror each evaluate a real component as a sum of four products, gamma_4 each -- and padding is exactly 0.  The shapes are the smallest
that take every path of the kernel: bonds 1, 2, 3, 8, 15, 16, 17 and 33 (odd column-block starts, the last b of an odd bond, chunk
tails, two and three chunks, w chi crossing multiples of 16), MPO bonds 1, 2, 3, 5 and 32 with 32 x 16 = 512, one site, an identity
site inside the support, a v and a u without a listed block."""
import functools
import os
import re
import sys

import numpy as np
import pytest

import qml_cutensornet_amd as Q
from helpers import canary_copy, scrambled
from qml_cutensornet_amd import engine
from qml_cutensornet_amd.engine import QkError
from test_matrix_gates_host import from_gates, haar
from test_mpo_host import heisenberg_terms, random_dense_mpo, term_bound
from test_projected_host import dense

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U53 = 2.0**-53
QK_EINVAL = -1  # include/qkgram.h


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------
def raw_mps(prof, rng):
    """Unit-scale complex tensors with the given bonds (no gauge, no norm: the product is elementwise)."""
    return Q.MPS([rng.uniform(-1, 1, (l, 2, r)) + 1j * rng.uniform(-1, 1, (l, 2, r)) for l, r in zip(prof, prof[1:])])


PROFILES9 = ([1, 2, 3, 8, 15, 16, 17, 33, 2, 1], [1, 1, 2, 17, 33, 16, 15, 3, 8, 1], [1, 16, 16, 3, 1, 2, 33, 33, 2, 1])
MPO_BONDS9 = [1, 2, 3, 5, 1, 1, 2, 3, 2, 1]


@functools.lru_cache(maxsize=None)
def main_case():
    """(states, Mpo) on 9 sites: three states of different bonds; MPO bonds 1, 2, 3, 5; site 4 is the exact identity between
    operators; site 2 has no block with v = 3, site 3 none with u = 1, and single blocks are zero (one as -0.0)."""
    rng = np.random.default_rng(900)
    states = tuple(raw_mps(p, rng) for p in PROFILES9)
    ts = [t.copy() for t in random_dense_mpo(rng, MPO_BONDS9).tensors]
    ts[4] = np.eye(2, dtype=complex).reshape(1, 1, 2, 2)
    ts[2][:, 3] = 0.0
    ts[3][1, :] = 0.0
    ts[1][1, 2], ts[6][0, 1], ts[7][2, 0] = 0.0, -0.0, 0.0
    return states, engine.Mpo(ts)


@functools.lru_cache(maxsize=None)
def w32_case():
    """MPO bond 32 on bonds 16 (exactly 512), 15 and 2."""
    rng = np.random.default_rng(901)
    return (raw_mps([1, 16, 16, 1], rng), raw_mps([1, 2, 15, 1], rng)), random_dense_mpo(rng, [1, 32, 32, 1])


@functools.lru_cache(maxsize=None)
def n1_case():
    rng = np.random.default_rng(902)
    return (raw_mps([1, 1], rng), raw_mps([1, 1], rng)), random_dense_mpo(rng, [1, 1])


CASES = {"main": main_case, "w32": w32_case, "n1": n1_case}


def image(s):
    """(planes, true bonds, offsets) of a device set."""
    nd, _, dims, offs = s.image()
    planes = np.empty(nd, dtype=np.float64)
    s.copy_image(planes.ctypes.data, nd)
    return planes, dims, offs


def host_image(states):
    return np.concatenate([engine.pack_state(m)[0] for m in states])


def state_images(s):
    planes, _, offs = image(s)
    cuts = [int(o[0]) for o in offs] + [planes.size]
    return [planes[a:b] for a, b in zip(cuts, cuts[1:])]


def bound_image(states, mpo):
    """8 u sum_s (|Re W| + |Im W|)(|Re A| + |Im A|) of every element, 0 on the padding, laid out as the product's image."""
    out = []
    for m in states:
        ts = []
        for W, A in zip(mpo.tensors, m.tensors):
            B = np.einsum("uvts,asb->uatvb", np.abs(W.real) + np.abs(W.imag), np.abs(A.real) + np.abs(A.imag))
            ts.append((B.reshape(W.shape[0] * A.shape[0], 2, W.shape[1] * A.shape[2]) * (1 + 1j)).astype(np.complex128))
        out.append(engine.pack_state(Q.MPS(ts))[0])
    return 8 * U53 * np.concatenate(out)


def apply_image(ctx, states, mpo):
    with ctx.upload(list(states)) as xs, ctx.apply_mpo(xs, mpo) as ps:
        return image(ps)


# ---- 1. elementwise against the mirror ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_elementwise_against_the_mirror(gpu_ctx, name):
    states, O = CASES[name]()
    with gpu_ctx.upload(list(states)) as xs:
        src = image(xs)[0]
        with gpu_ctx.apply_mpo(xs, O) as ps:
            planes, dims, offs = image(ps)
            assert ps.centre == -1 and ps.precision == 64
            assert np.array_equal(ps.dims, dims)
        assert np.array_equal(image(xs)[0], src)  # the source is untouched
    mirror = [m.apply_mpo(O) for m in states]
    assert np.array_equal(dims, np.stack([m.bond_dims() for m in mirror]))
    assert np.array_equal(dims, np.stack([O.bonds * m.bond_dims() for m in states]))
    want, bound = host_image(mirror), bound_image(states, O)
    assert planes.shape == want.shape == bound.shape
    assert np.array_equal(offs.reshape(-1), np.concatenate([[0], np.cumsum([4 * (-(-a // 16) * 16) * (-(-b // 16) * 16) for d in dims for a, b in zip(d, d[1:])])[:-1]]))
    err = np.abs(planes - want)
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(f"{name}: {planes.size} doubles, max bond {dims.max()}, max |dev - mirror| = {err.max():.3e}, max |d| / bound = {worst:.3f}")
    assert np.all(np.isfinite(planes))
    assert np.all(err <= bound)  # the padding and the zero blocks have bound 0: exactly 0 there
    if name == "w32":
        assert dims.max() == 512
    if name == "main":
        assert np.any((bound == 0) & (want == 0)) and int((want != 0).sum()) > planes.size // 8


# ---- 2. bits ---------------------------------------------------------------------------------------------------------------------
def test_a_product_is_the_same_bits_alone_in_any_set_in_any_order_and_again(gpu_ctx):
    states, O = main_case()
    with gpu_ctx.upload(list(states)) as xs, gpu_ctx.apply_mpo(xs, O) as ps:
        ref = state_images(ps)
    with gpu_ctx.upload(list(states)) as xs, gpu_ctx.apply_mpo(xs, O) as ps:
        again = state_images(ps)
    order = [2, 0, 1, 0]
    with gpu_ctx.upload([states[i] for i in order]) as xs, gpu_ctx.apply_mpo(xs, O) as ps:
        mixed = state_images(ps)
    for i in range(3):
        with gpu_ctx.upload([states[i]]) as xs, gpu_ctx.apply_mpo(xs, O) as ps:
            alone = state_images(ps)
        assert len(alone) == 1 and np.array_equal(alone[0], ref[i]) and np.array_equal(again[i], ref[i])
    for j, i in enumerate(order):
        assert np.array_equal(mixed[j], ref[i])


def test_the_identity_mpo_gives_the_source_image(gpu_ctx):
    states = main_case()[0]
    ident = engine.Mpo([np.eye(2).reshape(1, 1, 2, 2)] * 9)
    # signed zeros and a NaN-free source: a copy keeps the bits an arithmetic identity would not (-0.0 + 0.0 = +0.0)
    ts = [t.copy() for t in states[0].tensors]
    ts[3][0, 0, 0], ts[5][1, 1, 2] = complex(-0.0, 0.0), complex(0.0, -0.0)
    src = [Q.MPS(ts), states[1], states[2]]
    with gpu_ctx.upload(src) as xs, gpu_ctx.apply_mpo(xs, ident) as ps:
        a, b = image(xs), image(ps)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))  # bit for bit, signed zeros included


def test_doubling_one_tensor_doubles_exactly_that_site(gpu_ctx):
    states, O = main_case()
    k = 3
    O2 = engine.Mpo([t * 2 if j == k else t for j, t in enumerate(O.tensors)])
    p1, dims, offs = apply_image(gpu_ctx, states, O)
    p2, dims2, offs2 = apply_image(gpu_ctx, states, O2)
    assert np.array_equal(dims, dims2) and np.array_equal(offs, offs2)
    ends = np.append(offs.reshape(-1)[1:], p1.size).reshape(offs.shape)
    for s in range(len(states)):
        for j in range(9):
            a, b = p1[offs[s, j] : ends[s, j]], p2[offs[s, j] : ends[s, j]]
            assert np.array_equal(b, 2 * a if j == k else a)
    assert np.abs(p1[offs[0, k] : ends[0, k]]).max() > 0


def test_a_canary_spoils_its_own_product_only_and_a_zero_block_stays_zero(gpu_ctx):
    states, O = main_case()
    clean, dims, offs = apply_image(gpu_ctx, states, O)
    mixed = [states[0], canary_copy(states[1]), states[2]]
    with gpu_ctx.upload(mixed) as xs, gpu_ctx.apply_mpo(xs, O) as ps:
        got = state_images(ps)
        spoiled = ps.download()[1]
    cuts = [int(o[0]) for o in offs] + [clean.size]
    assert np.array_equal(got[0], clean[cuts[0] : cuts[1]]) and np.array_equal(got[2], clean[cuts[2] : cuts[3]])
    chi = PROFILES9[1]
    for k, (W, B) in enumerate(zip(O.tensors, spoiled.tensors)):
        l, r = chi[k], chi[k + 1]
        for u in range(W.shape[0]):
            for v in range(W.shape[1]):
                blk = B[u * l : (u + 1) * l, :, v * r : (v + 1) * r]
                if np.all(W[u, v] == 0):
                    assert np.all(blk == 0), (k, u, v)  # not read: exact zeros against a NaN source
                elif k == 4:
                    assert np.all(np.isnan(blk.real) & np.isnan(blk.imag))  # the copied site
                else:
                    assert np.all(np.isnan(blk.real) | np.isnan(blk.imag)), (k, u, v)
    unread = ~(bound_image([states[1]], O) > 0)  # the padding and the zero blocks, in the layout of the image
    assert np.all(got[1][unread] == 0) and np.all(np.isnan(got[1][~unread]))


# ---- 3. consumers ----------------------------------------------------------------------------------------------------------------
def unit_states(n, profs, seed):
    rng = np.random.default_rng(seed)
    return [scrambled(Q.random_mps(n, p, rng), rng) for p in profs]


@functools.lru_cache(maxsize=None)
def heis8():
    terms = heisenberg_terms(8)
    return engine.mpo_from_terms(8, terms), term_bound(terms)


PROF8 = ([1, 2, 4, 8, 16, 8, 4, 2, 1], [1, 2, 4, 7, 9, 8, 4, 2, 1], [1, 2, 3, 5, 6, 5, 4, 2, 1], [1, 2, 4, 8, 15, 8, 4, 2, 1])


def test_overlap_with_the_product_is_the_expectation_value(gpu_ctx):
    n = 12
    terms = heisenberg_terms(n)
    H, S = engine.mpo_from_terms(n, terms), term_bound(terms)
    profs = ([1, 2, 4, 8, 16, 32, 33, 17, 9, 5, 3, 2, 1], [1, 2, 4, 8, 15, 16, 16, 16, 8, 4, 2, 2, 1], [1, 2, 3, 3, 3, 3, 3, 3, 3, 3, 3, 2, 1])
    states = unit_states(n, profs, 910)
    with gpu_ctx.upload(states) as xs:
        V, nrm = gpu_ctx.mpo_expectations(xs, [H], norms=True)
        with gpu_ctx.apply_mpo(xs, H) as ox:
            assert ox.dims.max() == 5 * 33
            z = gpu_ctx.overlaps(xs, ox)
    got = np.diag(z) / nrm
    err = float(np.abs(got - V[:, 0]).max())
    print(f"<x|O x> / <x|x> against mpo_expectations: S = {S:.4g}, max |d| / S = {err / S:.3e}")
    assert np.abs(V).max() > 1e-3 and err <= 1e-12 * S


def test_operator_matrix(gpu_ctx):
    H, S = heis8()
    xs_h, ys_h = unit_states(8, PROF8, 911), unit_states(8, PROF8[:3], 912)
    Xd, Yd = np.stack([dense(m) for m in xs_h], axis=1), np.stack([dense(m) for m in ys_h], axis=1)
    Hd = H.to_dense()
    with gpu_ctx.upload(xs_h) as xs, gpu_ctx.upload(ys_h) as ys:
        M = gpu_ctx.operator_matrix(xs, H, ys)
        Msym = gpu_ctx.operator_matrix(xs, H)
        Mc = gpu_ctx.operator_matrix(xs, H, ys, max_discard=0.0)
        with pytest.raises(ValueError, match="info is not an argument"):
            gpu_ctx.operator_matrix(xs, H, info=True)
    assert M.shape == (3, 4) and M.dtype == np.complex128 and Msym.shape == (4, 4)
    e_rect, e_sym = float(np.abs(M - Yd.conj().T @ Hd @ Xd).max()), float(np.abs(Msym - Xd.conj().T @ Hd @ Xd).max())
    e_herm, e_c = float(np.abs(Msym - Msym.conj().T).max()), float(np.abs(Mc - M).max())
    print(f"operator_matrix: S = {S:.4g}, |d| / S = {e_rect / S:.3e} (rectangular), {e_sym / S:.3e} (square), {e_herm / S:.3e} (Hermitian), {e_c / S:.3e} (compressed)")
    assert e_rect <= 1e-12 * S and e_sym <= 1e-12 * S and e_herm <= 1e-12 * S
    assert e_c <= 1e-11 * S  # the compress sweep's own bound between a set and its max_discard = 0 twin (tests/test_gpu_compress.py)
    # a non-Hermitian operator: the MPO acts on the ket side, the conjugate is taken on ys
    G = engine.mpo_two_qubit_gate(8, 6, 1, haar(np.random.default_rng(5), 4))
    with gpu_ctx.upload(xs_h) as xs, gpu_ctx.upload(ys_h) as ys:
        Mg = gpu_ctx.operator_matrix(xs, G, ys)
    assert np.abs(Mg - Yd.conj().T @ G.to_dense() @ Xd).max() <= 1e-12 * 4


def test_compressed_products(gpu_ctx):
    H, _ = heis8()
    states = unit_states(8, PROF8, 913)
    P = engine.mpo_parity_projector(8, +1)
    with gpu_ctx.upload(states) as xs:
        ps, info = gpu_ctx.apply_mpo(xs, H, max_discard=0.0, info=True)
        with ps:
            assert set(info) == {"product_bond_dims", "fidelity", "discarded", "bond_dims"}
            assert np.array_equal(info["product_bond_dims"], H.bonds * xs.dims)
            assert np.all(info["bond_dims"] <= info["product_bond_dims"]) and np.any(info["bond_dims"] < info["product_bond_dims"])
            assert np.array_equal(ps.dims, info["bond_dims"])
            print(f"max_discard = 0: max |fidelity - 1| = {np.abs(info['fidelity'] - 1).max():.3e}, max bond {info['product_bond_dims'].max()} -> {info['bond_dims'].max()}")
            assert np.abs(info["fidelity"] - 1).max() <= 1e-12
        exact, only = gpu_ctx.apply_mpo(xs, H, info=True)
        exact.close()
        assert set(only) == {"product_bond_dims"}
        capped, cinfo = gpu_ctx.apply_mpo(xs, H, max_bond=4, info=True)
        capped.close()
        assert cinfo["bond_dims"].max() == 4 and np.all(cinfo["fidelity"] < 1)
        # parity twice, then compressed, against parity once
        with gpu_ctx.apply_mpo(xs, P) as p1, gpu_ctx.apply_mpo(p1, P, max_discard=0.0) as p2:
            assert np.array_equal(p1.dims, P.bonds * xs.dims) and np.all(p2.dims <= p1.dims)
            z12, z11, z22 = np.diag(gpu_ctx.overlaps(p1, p2)), np.diag(gpu_ctx.overlaps(p1)).real, np.diag(gpu_ctx.overlaps(p2)).real
    ov = np.abs(z12) / np.sqrt(z11 * z22)
    print(f"P P psi against P psi: max |normalised overlap - 1| = {np.abs(ov - 1).max():.3e}, weights {z11.min():.3f} .. {z11.max():.3f}")
    assert np.all(z11 > 0.05) and np.abs(ov - 1).max() <= 1e-10


def test_the_seeded_builder_takes_a_product(gpu_ctx):
    n = 8
    rng = np.random.default_rng(914)
    states = unit_states(n, PROF8[:3], 915)
    G = engine.mpo_two_qubit_gate(n, 1, 6, haar(rng, 4))
    circuit = from_gates(n, [("Unitary2q", [2, 3], [haar(rng, 4)]), ("Ry", [5], [0.3])])
    with gpu_ctx.upload(states) as xs, gpu_ctx.apply_mpo(xs, G) as ps, gpu_ctx.seed(ps, sweep=True) as seed:
        dev, _ = gpu_ctx.build_mps([circuit] * 3, initial=(seed, 0))
    for m, got in zip(states, dev):
        host = Q.simulate(circuit, 1 - 1e-16, initial=m.apply_mpo(G))
        x, y = dense(got), dense(host)
        ov = abs(np.vdot(y, x)) / (np.linalg.norm(x) * np.linalg.norm(y))
        assert abs(np.linalg.norm(x) - 1) <= 1e-10 and abs(ov - 1) <= 1e-10


# ---- 4. the driver ---------------------------------------------------------------------------------------------------------------
def sym_ansatz(n=8):
    """Ry(x_q) on every qubit, then two brick layers of XXPhase and a layer of Rx: a generic state mixes both parity sectors; x = 0
    gives a state in the even sector (XXPhase and ZZPhase keep the parity of |0...0>)."""
    gates = [("Ry", [q], (1.0, (q, 0.0, 1.0))) for q in range(n)]
    for layer in range(2):
        gates += [("XXPhase", [a, a + 1], (0.7, (a, 1.0, -1.0), (a + 1, 1.0, -1.0))) for a in range(layer % 2, n - 1, 2)]
        gates += [("ZZPhase", [a, a + 2], 0.3) for a in range(0, n - 2, 3)]
    return Q.CircuitAnsatz(n, gates)


def sym_points():
    rng = np.random.default_rng(916)
    return rng.uniform(-1, 1, (5, 8)), rng.uniform(-1, 1, (3, 8))


def dense_symmetrized(ans, P, X, Y=None):
    Pd = P.to_dense()
    px = [Pd @ dense(Q.simulate(ans.circuit_for_data(x), 1 - 1e-16)) for x in X]
    py = px if Y is None else [Pd @ dense(Q.simulate(ans.circuit_for_data(y), 1 - 1e-16)) for y in Y]
    wx, wy = np.array([np.vdot(v, v).real for v in px]), np.array([np.vdot(v, v).real for v in py])
    return np.abs(np.array([[np.vdot(b, a) for a in px] for b in py])) ** 2 / np.outer(wy, wx)


def _sym_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["QK_BUILDER"] = "host"
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from qml_cutensornet_amd.dist import TorchComm
        from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_symmetrized_kernel_matrix

        X, Y = sym_points()
        P = engine.mpo_parity_projector(8, -1)
        comm = TorchComm()
        out = {"sym": build_symmetrized_kernel_matrix(comm, sym_ansatz(), X, projector=P, truncation_error=1e-16),
               "rect": build_symmetrized_kernel_matrix(comm, sym_ansatz(), X, Y, projector=P, truncation_error=1e-16)}
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_symmetrized_kernel_against_dense_vectors(gpu_ctx):
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_symmetrized_kernel_matrix

    ans, (X, Y) = sym_ansatz(), sym_points()
    for sign in (+1, -1):
        P = engine.mpo_parity_projector(8, sign)
        K = build_symmetrized_kernel_matrix(SingleComm(), ans, X, projector=P, truncation_error=1e-16)
        Kr = build_symmetrized_kernel_matrix(SingleComm(), ans, X, Y, projector=P, truncation_error=1e-16)
        ref, ref_r = dense_symmetrized(ans, P, X), dense_symmetrized(ans, P, X, Y)
        print(f"sign {sign:+d}: max |dK| = {np.abs(K - ref).max():.3e} (symmetric), {np.abs(Kr - ref_r).max():.3e} (rectangular); off-diagonal {np.abs(ref - np.eye(5)).max():.3f}")
        assert K.shape == (5, 5) and Kr.shape == (3, 5)
        assert np.abs(K - ref).max() <= 1e-10 and np.abs(Kr - ref_r).max() <= 1e-10
        assert np.array_equal(K, K.T) and np.abs(np.diag(K) - 1).max() <= 1e-10
        assert 0.01 < np.abs(ref - np.eye(5)).max() < 0.99
    # a cap that truncates changes K by little, and the arguments are checked
    Kc = build_symmetrized_kernel_matrix(SingleComm(), ans, X, projector=P, truncation_error=1e-16, max_bond=3)
    assert Kc.shape == (5, 5) and np.abs(Kc - K).max() > 0 and np.all(np.isfinite(Kc))
    # a data point outside the sector: x = 0 is an even state
    Xz = X.copy()
    Xz[3] = 0.0
    with pytest.raises(ValueError, match=r"data point 3 of X has weight .* <= min_weight"):
        build_symmetrized_kernel_matrix(SingleComm(), ans, Xz, projector=engine.mpo_parity_projector(8, -1), truncation_error=1e-16)
    with pytest.raises(ValueError, match=r"data point 1 of Y"):
        build_symmetrized_kernel_matrix(SingleComm(), ans, X, Xz[2:4], projector=engine.mpo_parity_projector(8, -1), truncation_error=1e-16)
    Ke = build_symmetrized_kernel_matrix(SingleComm(), ans, Xz, projector=engine.mpo_parity_projector(8, +1), truncation_error=1e-16)
    assert np.abs(Ke - dense_symmetrized(ans, engine.mpo_parity_projector(8, +1), Xz)).max() <= 1e-10
    for kwargs, match in ((dict(projector=None), "engine.Mpo"), (dict(projector=engine.mpo_parity_projector(7)), "7 sites"),
                          (dict(projector=P, truncation_error=None), "truncation error"), (dict(projector=P, min_weight=-1.0), "min_weight")):
        with pytest.raises(ValueError, match=match):
            build_symmetrized_kernel_matrix(SingleComm(), ans, X, **{"truncation_error": 1e-16, **kwargs})


@pytest.mark.timeout(300)
def test_symmetrized_kernel_one_and_two_ranks_give_the_same_bits(gpu_ctx, monkeypatch):
    import torch.multiprocessing as mp

    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_symmetrized_kernel_matrix

    ans, (X, Y) = sym_ansatz(), sym_points()
    P = engine.mpo_parity_projector(8, -1)
    monkeypatch.setenv("QK_BUILDER", "host")
    one = {"sym": build_symmetrized_kernel_matrix(SingleComm(), ans, X, projector=P, truncation_error=1e-16),
           "rect": build_symmetrized_kernel_matrix(SingleComm(), ans, X, Y, projector=P, truncation_error=1e-16)}
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + ((os.getpid() + 977) % 2000)
    procs = [ctx.Process(target=_sym_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert res[1]["sym"] is None and res[1]["rect"] is None
    assert np.array_equal(res[0]["sym"], one["sym"]) and np.array_equal(res[0]["rect"], one["rect"])


# ---- 5. rejections ---------------------------------------------------------------------------------------------------------------
def test_every_rejection(gpu_ctx):
    import ctypes as C

    L = engine.lib()
    rng = np.random.default_rng(917)
    states = [raw_mps([1, 2, 16, 2, 1], rng), raw_mps([1, 2, 19, 2, 1], rng)]
    O = random_dense_mpo(rng, [1, 2, 3, 2, 1])

    def call(ctx, xs, bonds, tensors, out=True):
        h = C.c_void_p()
        b = None if bonds is None else np.ascontiguousarray(bonds, dtype=np.int32)
        t = None if tensors is None else np.ascontiguousarray(tensors, dtype=np.float64)
        rc = L.qk_mps_set_apply_mpo(ctx, xs, None if b is None else b.ctypes.data, None if t is None else t.ctypes.data, C.byref(h) if out else None)
        assert h.value is None
        return rc, L.qk_last_error().decode()

    with gpu_ctx.upload(states) as xs:
        good = (gpu_ctx.handle, xs.handle, O.bonds, O.packed())
        for k, name in ((0, "ctx"), (1, "src"), (2, "bonds"), (3, "tensors")):
            rc, msg = call(*[None if j == k else a for j, a in enumerate(good)])
            assert rc == QK_EINVAL and f"qk_mps_set_apply_mpo: {name} is null" in msg
        rc, msg = call(*good, out=False)
        assert rc == QK_EINVAL and "out is null" in msg
        with engine.Context(0) as other:
            with pytest.raises(QkError, match="set belongs to another context"):
                other.apply_mpo(xs, O)
        with xs.to_f32() as x32:
            with pytest.raises(QkError, match="complex64"):
                gpu_ctx.apply_mpo(x32, O)
        for bonds, match in (([1, 2, 0, 2, 1], r"bonds\[2\] = 0 is outside 1 \.\. 32 \(cut 2\)"), ([1, 2, 33, 2, 1], r"bonds\[2\] = 33 is outside 1 \.\. 32 \(cut 2\)")):
            rc, msg = call(gpu_ctx.handle, xs.handle, bonds, np.zeros(8 * 33 * 4))
            assert rc == QK_EINVAL and re.search(match, msg), msg
        for bonds, match in (([2, 2, 3, 2, 1], "bonds[0] = 2 must be 1"), ([1, 2, 3, 2, 2], "bonds[4] = 2 must be 1")):
            rc, msg = call(gpu_ctx.handle, xs.handle, bonds, np.zeros(8 * 33 * 4))
            assert rc == QK_EINVAL and match in msg, msg
        for bad in (np.nan, np.inf):
            t = O.packed().copy()
            t[8 * 2 + 8 * (1 * 3 + 2) + 4 * 1 + 2 * 0 + 1] = bad  # site 1, W[1][2][1][0], imaginary part
            rc, msg = call(gpu_ctx.handle, xs.handle, O.bonds, t)
            assert rc == QK_EINVAL and "site 1: W[1][2][1][0] has a imaginary part that is not finite" in msg, msg
        # 19 x 27 = 513 is refused by name; 16 x 32 = 512 is taken
        big = random_dense_mpo(rng, [1, 2, 27, 2, 1])
        with pytest.raises(QkError, match=r"state 1, bond 2: the product bond 27 x 19 = 513 is above 512"):
            gpu_ctx.apply_mpo(xs, big)
    with gpu_ctx.upload(states[:1]) as xs, gpu_ctx.apply_mpo(xs, random_dense_mpo(rng, [1, 2, 32, 2, 1])) as ps:
        assert ps.dims.max() == 512
    with gpu_ctx.upload(states) as xs:
        with pytest.raises(ValueError, match="takes one Mpo"):
            gpu_ctx.apply_mpo(xs, [O])
        with pytest.raises(ValueError, match="has 5 sites, the states have 4"):
            gpu_ctx.apply_mpo(xs, engine.mpo_parity_projector(5))
