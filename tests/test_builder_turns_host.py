"""CPU tier of tests/test_gpu_builder_turns.py: the cases of ``helpers.BUILDER_TURN_SETS`` are what the GPU tests take them for -- with
the host builder alone.  A case holds slots + 40 states, slots = workgroups per CU x CUs; here the CUs of a 256-CU part (the GPU tests
read the slots from a probe build).  Asserted: the queue's proxies are distinct, so the queue order is known; the states that come on
a later turn -- the lightest in the default order, the last ones under QK_BUILD_NO_ORDER -- reach the bonds at which the builder
takes its block paths; the partial case has states that outgrow its cap and states that do not on both sides of the first turn;
and the truncating case loses fidelity on the first turn."""
import numpy as np
import pytest

import helpers as H

NUM_CUS = 256


@pytest.fixture(scope="module")
def cases(built):
    out = {}
    for name, (n, _, _, max_bond, _, per_cu, _, _) in H.BUILDER_TURN_SETS.items():
        slots = per_cu * NUM_CUS
        circuits = H.builder_turn_circuits(name, slots)
        out[name] = (slots, circuits, H.host_states(circuits))
    return out


@pytest.mark.parametrize("name", list(H.BUILDER_TURN_SETS))
def test_queue_order_is_known(cases, name):
    slots, circuits, _ = cases[name]
    assert len(circuits) == slots + H.BUILDER_TURN_EXTRA
    proxy = np.array([H.queue_proxy(c) for c in circuits])
    assert len(set(proxy.tolist())) == len(proxy) and np.diff(np.sort(proxy)).min() > 1e-9  # distinct beyond the rounding of a sum of sines
    order = H.queue_order(circuits)
    assert np.all(np.diff(proxy[order]) < 0) and sorted(order.tolist()) == list(range(len(circuits)))
    later = H.later_turn_states(circuits, slots)
    assert len(later) == H.BUILDER_TURN_EXTRA and proxy[later].max() < proxy[order[:slots]].min()  # the lightest states come on the later turns
    up = H.ascending_by_proxy(circuits)
    assert np.array_equal(up, order[::-1])
    assert np.array_equal(H.later_turn_states([circuits[i] for i in up], slots, ordered=False), np.arange(slots, len(circuits)))  # the heaviest come last


@pytest.mark.parametrize("name", list(H.BUILDER_TURN_SETS))
def test_later_turn_states_reach_the_block_paths(cases, name):
    n, _, _, max_bond, _, _, _, reach = H.BUILDER_TURN_SETS[name]
    slots, circuits, host = cases[name]
    bonds = np.array([m.max_bond() for m in host])
    later = H.later_turn_states(circuits, slots)
    print(f"{name}: {len(circuits)} states, bonds {bonds.min()}..{bonds.max()}, of the later-turn states {bonds[later].min()}..{bonds[later].max()}")
    assert bonds.max() <= max_bond and all(abs(m.fidelity - 1) < 1e-12 for m in host)  # nothing outgrows the cap, nothing is truncated
    assert bonds[later].max() >= reach  # default order: the later-turn states are the lightest, and still reach the block paths
    up = H.ascending_by_proxy(circuits)
    assert bonds[up[slots:]].max() >= reach and bonds[up[slots:]].max() == bonds.max()  # ascending order: the heaviest states are the later-turn ones
    assert bonds[up[:slots]].min() < bonds[up[slots:]].max()  # ... on arenas that held lighter ones


def test_partial_case_mixes_dropped_and_ordinary_states(built):
    """by the largest bond a state reaches at any gate, which is what drops it on the device"""
    name, _, per_cu, _, cap, least = H.BUILDER_TURN_PARTIAL
    slots = per_cu * NUM_CUS
    circuits = H.builder_turn_circuits(name, slots)
    host = H.host_states(circuits)
    final = np.array([m.max_bond() > cap for m in host])
    above = H.outgrows(circuits, cap, host)
    assert np.all(above[final]) and (above & ~final).sum() >= 1  # some states outgrow the cap on the way only
    for what, later in (("default order", H.later_turn_states(circuits, slots)), ("ascending order", H.ascending_by_proxy(circuits)[slots:])):
        first = np.setdiff1d(np.arange(len(circuits)), later)
        print(f"partial case, {what}: outgrow the cap {int(above[first].sum())} of the first {slots} ({int(final[first].sum())} by their final bonds), "
              f"{int(above[later].sum())} of the {len(later)} on a later turn ({int(final[later].sum())})")
        assert above[later].sum() >= least and above[first].sum() >= least
        if what == "default order":  # droppers first, then dropped and ordinary states alike on the workgroups that held them
            assert (~above[later]).sum() >= least
        else:  # the other way round: ordinary states among the first, the heaviest states -- droppers mostly -- after them
            assert (~above[first]).sum() >= least and (~above[later]).sum() >= 1


def test_truncating_case_loses_fidelity_on_the_first_turn(cases):
    name, cap, share, least = H.BUILDER_TURN_TRUNCATE
    slots, circuits, free = cases[name]
    host = H.host_states(circuits, max_bond=cap)
    cut = np.array([m.fidelity < 1 - 1e-6 for m in host])
    later = H.later_turn_states(circuits, slots)
    first = np.setdiff1d(np.arange(len(circuits)), later)
    print(f"truncating case at bond {cap}: {int(cut[first].sum())} of the first {slots} and {int(cut[later].sum())} of the {len(later)} later-turn states below 1 - 1e-6, "
          f"lowest fidelity {min(m.fidelity for m in host):.4f}")
    assert max(m.max_bond() for m in host) == cap < min(m.max_bond() for m in free)
    assert cut[first].sum() >= share * slots and cut[later].sum() >= least and (~cut[later]).sum() >= least


def test_launch_record_is_bound(built):
    """``qk_built_launch``, the accessor the GPU tests read their precondition from: exported, bound, and a null handle is an error"""
    from qml_cutensornet_amd import engine

    assert "qk_built_launch" in engine.EXPORTED_SYMBOLS and hasattr(engine.lib(), "qk_built_launch")
    assert engine.lib().qk_built_launch(None, None, None, None) != 0
