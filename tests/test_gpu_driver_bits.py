"""Every driver of ``gpu_backend/kernel_state_ansatz.py`` returns the bits, and writes the profile keys, of the commit before the
drivers were folded onto shared helpers (the run prologue, the share loop, the exchange, the profile writer).

tests/golden/drivers_parent_bits.json was recorded once on an MI355X at that parent commit by running this module as a script,
``python tests/test_gpu_driver_bits.py tests/golden/drivers_parent_bits.json``: for every case of ``CASES`` the SHA-1 of each
returned array (dict and tuple results flattened, dicts in sorted key order; shape and dtype enter the digest) and, where the driver
takes ``info_file``, the ordered (key, unit) pairs of its JSON.  Two recordings at the parent were identical in every case, so every
case is compared exactly.  6 qubits, 2 layers, X of 5 points, Y of 3, one rank, ``QK_BUILDER=device``: the smallest shapes that
reach every branch of the drivers, with the host / device builder policy kept out of the comparison (the device builder's own bits
are pinned across commits by the other golden files).
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "drivers_parent_bits.json")
N, LAYERS, NX, NY = 6, 2, 5, 3


def _inputs():
    import qml_cutensornet_amd as Q
    from oracle import restatement as R
    from qml_cutensornet_amd import engine
    from test_feature_map_host import zz_template

    rng = np.random.default_rng(68)
    return {
        "ans": Q.KernelStateAnsatz(N, LAYERS, 1.0, Q.entanglement_graph(N, 2)),
        "noisy": Q.CircuitAnsatz(N, engine.with_noise(zz_template(N, LAYERS, 0.8, 2), "AmplitudeDamping", [0.05], after="two_qubit")),
        "X": R.synthetic_features(NX, N, 13),
        "Y": R.synthetic_features(NY, N, 14),
        "strings": ["ZIIIII", "IXXIII", ("ZYZ", (2, 3, 5)), "XYZXYZ"],
        "mpo": engine.mpo_exponential(N, "Z", "Z", 1.0, 0.7),
        "projector": engine.mpo_parity_projector(N, -1),
        "bits": rng.integers(0, 2, size=(7, N)).astype(np.uint8),
        "own_bits": rng.integers(0, 2, size=(NX, 7, N)).astype(np.uint8),
        "bases": engine.random_bases(7, N, 21),
        "partial": np.where(rng.random((7, N)) < 0.5, rng.integers(1, 4, size=(7, N)), 0).astype(np.uint8),
        "seeds": [Q.random_mps(N, [1, 2, 3, 4, 3, 2, 1], rng) for _ in range(NX)],
    }


# name: (driver, takes Y, takes info_file, keyword arguments; a str value names an entry of ``_inputs``)
CASES = {
    "kernel": ("build_kernel_matrix", True, True, {}),
    "kernel-initial": ("build_kernel_matrix", True, True, {"initial_states": "seeds", "initial_states_Y": "seed0"}),
    "projected": ("build_projected_kernel_matrix", True, True, {}),
    "projected-pairs": ("build_projected_kernel_matrix", True, True, {"rdm": 2, "pair_distance": 2}),
    "projected-window": ("build_projected_kernel_matrix", True, True, {"rdm": 3, "window": True}),
    "projected-strings": ("build_projected_kernel_matrix", True, True, {"observables": "strings"}),
    "projected-mpo": ("build_projected_kernel_matrix", True, True, {"observables": "one_mpo"}),
    "projected-shots": ("build_projected_kernel_matrix", True, True, {"shots": 8, "shot_seed": 5}),
    "projected-initial": ("build_projected_kernel_matrix", True, True, {"initial_states": "seed0", "initial_states_Y": "seed0"}),
    "shot-feature-strings": ("build_shot_feature_kernel_matrix", True, True, {"observables": "strings", "shots": 16, "shot_seed": 5}),
    "shot-feature-window": ("build_shot_feature_kernel_matrix", True, True, {"window": 2, "shots": 16, "shot_seed": 5, "settings": "window"}),
    "entanglement": ("build_entanglement_profile", False, True, {}),
    "likelihoods": ("build_outcome_likelihoods", False, False, {"bits": "bits", "bases": "bases"}),
    "likelihoods-per-state": ("build_outcome_likelihoods", False, False, {"bits": "own_bits", "bases": "bases", "per_state": True}),
    "marginals": ("build_outcome_marginals", False, False, {"bits": "bits", "bases": "partial"}),
    "mpo": ("build_mpo_expectations", False, False, {"mpos": "mpos"}),
    "capped": ("build_capped_kernel_matrices", True, True, {"caps": (2, 4)}),
    "symmetrized": ("build_symmetrized_kernel_matrix", True, False, {"projector": "projector"}),
    "block": ("build_block_kernel_matrices", True, True, {"widths": (1, 3, 6)}),
    "block-shots": ("build_block_kernel_matrices", True, True, {"widths": (1, 3, 6), "shots": (2, 4), "shot_seed": 5}),
    "shadow": ("build_shadow_kernel_matrix", True, True, {"shots": 8, "shot_seed": 5, "return_hist": True}),
    "depth-scan": ("build_depth_scan_kernel_matrices", True, True, {"depths": (1, 2)}),
    "noisy-projected": ("build_noisy_projected_kernel_matrix", True, False, {"trajectories": 2, "noise_seed": 5}),
    "noisy-projected-pairs": ("build_noisy_projected_kernel_matrix", True, False, {"trajectories": 2, "noise_seed": 5, "rdm": 2, "pair_distance": 2, "initial_states": "seed0"}),
    "noisy-kernel": ("build_noisy_kernel_matrix", True, False, {"trajectories": 2, "noise_seed": 5}),
}


def _flatten(path, value, out):
    """(path, SHA-1) of every array of a result: dicts in sorted key order, tuples and lists that hold arrays or dicts by position."""
    if isinstance(value, dict):
        for key in sorted(value, key=str):
            _flatten(f"{path}/{key}", value[key], out)
    elif isinstance(value, (tuple, list)) and any(isinstance(v, (dict, np.ndarray)) for v in value):
        for k, v in enumerate(value):
            _flatten(f"{path}/{k}", v, out)
    elif value is None:
        out.append([path, "None"])
    else:
        a = np.ascontiguousarray(value)
        out.append([path, hashlib.sha1(f"{a.dtype.str}{a.shape}".encode() + a.tobytes()).hexdigest()])


def run_case(name, tmp_dir, inputs=None):
    """{"sym" | "xy": {"digests": [[path, sha1], ...], "profile": [[key, unit], ...] or None}} of one case (needs a GPU)."""
    from qml_cutensornet_amd.dist import SingleComm
    from qml_cutensornet_amd.gpu_backend import kernel_state_ansatz as K

    inp = dict(_inputs() if inputs is None else inputs)
    inp.update(seed0=inp["seeds"][0], one_mpo=[inp["mpo"]], mpos=[inp["mpo"], inp["projector"]])
    driver, takes_y, takes_info, kwargs = CASES[name]
    kwargs = {k: (inp[v] if isinstance(v, str) and v in inp else v) for k, v in kwargs.items()}
    ans = inp["noisy"] if name.startswith("noisy") else inp["ans"]
    out = {}
    for form in ("sym", "xy") if takes_y else ("sym",):
        kw = dict(kwargs, truncation_error=1e-16)
        if form == "xy":
            kw["Y"] = inp["Y"]
        else:
            kw.pop("initial_states_Y", None)
        info = os.path.join(str(tmp_dir), f"{name}-{form}")
        if takes_info:
            kw["info_file"] = info
        digests = []
        _flatten("", getattr(K, driver)(SingleComm(), ans, inp["X"], **kw), digests)
        profile = None
        if takes_info:
            with open(info + ".json") as fp:
                profile = [[key, value[1]] for key, value in json.load(fp).items()]
        out[form] = {"digests": digests, "profile": profile}
    return out


@pytest.fixture(scope="module")
def driver_inputs(built):
    return _inputs()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_driver_returns_the_bits_and_profile_keys_of_the_parent(built, driver_inputs, monkeypatch, tmp_path, name):
    monkeypatch.setenv("QK_BUILDER", "device")
    with open(FIXTURE) as fp:
        want = json.load(fp)
    assert sorted(want) == sorted(CASES)
    got = run_case(name, tmp_path, driver_inputs)
    for form, rec in got.items():
        for (path, sha), (wpath, wsha) in zip(rec["digests"], want[name][form]["digests"]):
            print(f"{name} {form} {path}: {sha} {'==' if sha == wsha else '!='} {wsha}")
    assert got == want[name]


if __name__ == "__main__":  # the recorder: python tests/test_gpu_driver_bits.py OUT.json
    import tempfile

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["QK_BUILDER"] = "device"
    import __graft_entry__ as g

    g.build()
    with tempfile.TemporaryDirectory() as tmp:
        shared = _inputs()
        recorded = {case: run_case(case, tmp, shared) for case in CASES}
    with open(sys.argv[1], "w") as fp:  # one line per case
        fp.write("{\n" + ",\n".join(f"{json.dumps(case)}: {json.dumps(rec)}" for case, rec in recorded.items()) + "\n}\n")
