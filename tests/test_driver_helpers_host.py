"""The helpers the drivers of ``gpu_backend/kernel_state_ansatz.py`` share, on the CPU: the chunk arithmetic, the run prologue and
the per-share feature loop.  No device: ``engine.device_count`` / ``engine.default_context`` and ``_simulate_share`` are replaced."""
import numpy as np
import pytest

from qml_cutensornet_amd import engine
from qml_cutensornet_amd.gpu_backend import kernel_state_ansatz as K


@pytest.mark.parametrize("n,n_procs", [(0, 3), (2, 5), (12, 4), (13, 4), (1, 1), (7, 2)])
def test_chunk_is_contiguous_ceil_chunks(n, n_procs):
    per_rank = -(-n // n_procs)  # ceil(n / n_procs)
    covered = []
    for rank in range(n_procs):
        lo, hi = K._chunk(n, rank, n_procs)
        assert (lo, hi) == (min(n, rank * per_rank), min(n, min(n, rank * per_rank) + per_rank))
        covered += list(range(lo, hi))
    assert covered == list(range(n))
    if n < n_procs:  # the trailing ranks hold nothing
        assert all(K._chunk(n, rank, n_procs) == (n, n) for rank in range(n, n_procs))


class _Comm:
    def __init__(self, rank, size):
        self.rank, self.size = rank, size

    def Get_rank(self):
        return self.rank

    def Get_size(self):
        return self.size


def test_start_without_a_device_names_the_driver(monkeypatch):
    def no_context(*a, **k):
        raise AssertionError("a context without a device")

    monkeypatch.setattr(engine, "device_count", lambda: 0)
    monkeypatch.setattr(engine, "default_context", no_context)
    with pytest.raises(engine.QkError, match="no gfx950 device visible: outcome likelihoods have no CPU fallback"):
        K._start(_Comm(0, 1), "outcome likelihoods have")


def test_start_places_rank_1_of_2_on_device_1_of_3(monkeypatch):
    sentinel, asked = object(), []
    monkeypatch.setattr(engine, "device_count", lambda: 3)
    monkeypatch.setattr(engine, "default_context", lambda device_id=0: asked.append(device_id) or sentinel)
    run = K._start(_Comm(1, 2), "the Gram path has")
    assert (run.rank, run.n_procs, run.device_id, run.is_root) == (1, 2, 1, False)
    assert run.ctx is sentinel and asked == [1] and run.host_workers >= 1 and run.t_start > 0
    with pytest.raises(AttributeError):
        run.rank = 0  # the record is immutable


class _Ctx:
    trims = 0

    def trim(self):
        self.trims += 1


class _Set:
    dims = np.array([[1, 2, 4, 2, 1], [1, 2, 3, 2, 1]], dtype=np.int32)
    closed = 0

    def close(self):
        self.closed += 1


def _run(ctx):
    return K._Run(rank=0, n_procs=1, is_root=False, device_id=0, host_workers=1, ctx=ctx, t_start=0.0)


def test_share_features_of_an_empty_share(monkeypatch):
    called = []
    monkeypatch.setattr(K, "_simulate_share", lambda *a, **k: (4, None, [], []))
    ctx = _Ctx()
    F, lo, chi, secs, fids, feat_secs = K._share_features(_run(ctx), None, np.zeros((4, 3)), "X", 1.0, (6, 3), lambda local, lo: called.append(lo))
    assert F.shape == (0, 6, 3) and F.dtype == np.float64 and not called
    assert lo == 4 and chi.shape == (0,) and secs == [] and fids == [] and feat_secs >= 0.0 and ctx.trims == 1


def test_share_features_closes_the_share_when_the_features_fail(monkeypatch):
    share = _Set()
    monkeypatch.setattr(K, "_simulate_share", lambda *a, **k: (0, share, [0.1, 0.1], [1.0, 1.0]))

    def features_of(local, lo):
        raise RuntimeError("the feature call failed")

    with pytest.raises(RuntimeError, match="the feature call failed"):
        K._share_features(_run(_Ctx()), None, np.zeros((2, 3)), "X", 1.0, (3,), features_of)
    assert share.closed == 1


def test_share_features_returns_the_features_and_the_largest_bonds(monkeypatch):
    share = _Set()
    monkeypatch.setattr(K, "_simulate_share", lambda *a, **k: (2, share, [0.1, 0.2], [1.0, 0.5]))
    F, lo, chi, secs, fids, _ = K._share_features(_run(_Ctx()), None, np.zeros((4, 3)), "Y", 1.0, (3,), lambda local, lo: np.full((2, 3), float(lo)))
    assert np.array_equal(F, np.full((2, 3), 2.0)) and lo == 2 and list(chi) == [4, 3] and secs == [0.1, 0.2] and fids == [1.0, 0.5]
    assert share.closed == 1
