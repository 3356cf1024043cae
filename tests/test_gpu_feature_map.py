"""GPU tests of custom feature maps: the device builder on Rx / Ry / YYPhase / ZZPhase programs against the host builder,
``build_kernel_matrix`` with a ``CircuitAnsatz`` and with a gate-list ansatz against exact state vectors, and the
rejection of unknown op codes by the device builder.

Tolerances as tests/test_gpu_builder.py: |<dev|host>|^2 = 1 within 1e-10, Gram entries of the two state sets within 1e-9;
Grams against the exact state vector within 1e-10."""
import numpy as np
import pytest

from oracle import restatement as R
from test_feature_map_host import GateListAnsatz, dense, exact, zz_template  # noqa: F401  (exact: fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("wgs", ["1", "2"])
@pytest.mark.parametrize("n,layers,gamma,nn,npts,big", [(10, 2, 1.0, 1, 5, False), (12, 2, 0.8, 3, 4, False), (16, 3, 0.5, 2, 4, True)])
def test_device_builder_matches_host_builder_on_feature_maps(gpu_ctx, monkeypatch, wgs, n, layers, gamma, nn, npts, big):
    import qml_cutensornet_amd as Q

    monkeypatch.setenv("QK_BUILD_WGS", wgs)
    ca = Q.CircuitAnsatz(n, zz_template(n, layers, gamma, nn))
    circuits = [ca.circuit_for_data(x) for x in R.synthetic_features(npts, n, 17)]
    assert {4, 5, 6, 7} <= set(circuits[0].op.tolist())
    dev, info = gpu_ctx.build_mps(circuits)
    host = [Q.simulate(c, 1 - 1e-16) for c in circuits]
    assert info["kernel_ms"] > 0 and len(dev) == npts
    if big:  # the MFMA theta product (bond >= 32) and the preconditioned block factorisations (>= 48 columns) ran
        assert max(m.max_bond() for m in host) > 64 and max(m.max_bond() for m in dev) > 64
    for md, mh in zip(dev, host):
        assert md.bond_dims()[0] == 1 and md.bond_dims()[-1] == 1
        assert abs(md.fidelity - 1.0) < 1e-12
    z = np.array([R.mps_inner(md.tensors, mh.tensors) for md, mh in zip(dev, host)])
    assert np.abs(np.abs(z) ** 2 - 1).max() < 1e-10
    with gpu_ctx.upload(dev) as dx, gpu_ctx.upload(host) as hx:
        assert np.abs(gpu_ctx.gram(dx) - gpu_ctx.gram(hx)).max() < 1e-9


def _gram_exact(exact, gl, X, Y):
    sx = [exact(gl.ansatz_circ.n_qubits, gl.circuit_for_data(x)) for x in X]
    sy = sx if Y is None else [exact(gl.ansatz_circ.n_qubits, gl.circuit_for_data(y)) for y in Y]
    return np.array([[abs(np.vdot(a, b)) ** 2 for a in sx] for b in sy])


@pytest.mark.parametrize("builder", ["device", "host"])
@pytest.mark.parametrize("as_gate_list", [False, True])
def test_build_kernel_matrix_with_feature_maps(built, exact, monkeypatch, builder, as_gate_list):
    import qml_cutensornet_amd as Q
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_kernel_matrix

    monkeypatch.setenv("QK_BUILDER", builder)
    n = 12
    tmpl = zz_template(n, 2, 0.7, 2)
    gl = GateListAnsatz(n, tmpl)
    ans = gl if as_gate_list else Q.CircuitAnsatz(n, tmpl)
    X, Y = R.synthetic_features(7, n, 31), R.synthetic_features(4, n, 32)
    K = build_kernel_matrix(SingleComm(), ans, X=X, truncation_error=1e-16)
    assert K.shape == (7, 7) and np.abs(K - _gram_exact(exact, gl, X, None)).max() < 1e-10
    Kt = build_kernel_matrix(SingleComm(), ans, X=X, Y=Y, truncation_error=1e-16)
    assert Kt.shape == (4, 7) and np.abs(Kt - _gram_exact(exact, gl, X, Y)).max() < 1e-10


def test_forced_device_builder_refuses_circuits_of_different_structure(built, monkeypatch):
    """Gate lists whose routing depends on the data point: one share, two structures -- a forced device build raises."""
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.engine import QkError
    from qml_cutensornet_amd.gpu_backend.kernel_state_ansatz import build_kernel_matrix

    class DataRouted(GateListAnsatz):
        def circuit_for_data(self, x):
            far = 3 if x[0] > 0 else 1
            return [("H", [q], []) for q in range(4)] + [("ZZPhase", [0, far], [float(x[1])])]

    X = np.array([[0.5, 0.3, 0, 0], [-0.5, 0.2, 0, 0], [0.1, 0.9, 0, 0]])
    monkeypatch.setenv("QK_BUILDER", "device")
    with pytest.raises(QkError, match="structure"):
        build_kernel_matrix(SingleComm(), DataRouted(4, []), X=X, truncation_error=1e-16)


@pytest.mark.parametrize("code", [8, -1])
def test_device_builder_rejects_unknown_op_codes(gpu_ctx, code):
    from qml_cutensornet_amd.ansatz import BoundCircuit
    from qml_cutensornet_amd.engine import QkError

    c = BoundCircuit(4, np.array([0, 0, 0, 0, code, 2], dtype=np.int8), np.array([0, 1, 2, 3, 1, 0], dtype=np.int32), np.array([0, 0, 0, 0, 0.6, 0.3]))
    with pytest.raises(QkError, match="op code"):
        gpu_ctx.build_mps([c, c])
