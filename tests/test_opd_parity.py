"""``plan_opd`` against the yardstick (tests/opd_util.py: restate_opd), exactly: the action, the greedy sequence, the expansions
made and the bits of value / upper, on the CPU emulation of the kernel source and, marked ``gpu``, on the MI355X.

1. The smallest shapes that can go wrong: E = 3, 8 traffic vehicles, 3 lanes, highway-fast's frequencies; one expansion, three,
   seventeen (86 nodes: the second lane pass), the longitudinal-only table, a DiscreteAction 3 x 3 table (stored controls travel
   through gather and scatter), Linear traffic, the Lidar observation.
2. Terminal leaves, solved trees and ties happen.  The seeds were chosen on the emulator:
   * ``dense`` (vehicles_density 3, seed 1): crashes within the first steps -- 14, 17 and 5 terminal nodes in the three trees;
   * ``short`` (duration 2, seed 2): every depth-2 node is truncated, the root and its five children are expanded and the sixth
     selection meets a done leaf: expanded == 6 < X == 17 in all three trees, and value == upper to the bit;
   * ``lane0`` (initial_lane_id 0, seed 1): LANE_LEFT does what IDLE does, to the bit -- a selection of environment 0 finds two
     leaves holding the largest upper."""
import numpy as np
import pytest

from tests import opd_util as ou

LINEAR = "highway_env.vehicle.behavior.LinearVehicle"
GAMMA = 0.7
# name: (config, budget, seed, warm-up actions)
SHAPES = {
    "b5_one_expansion": (ou.fast_config(8), 5, 11, ()),
    "b15_three_expansions": (ou.fast_config(8), 15, 11, ()),
    "b85_second_lane_pass": (ou.fast_config(8), 85, 11, ()),
    "b9_longitudinal_only": (ou.fast_config(8, action={"type": "DiscreteMetaAction", "lateral": False}), 9, 12, ()),
    "b27_discrete_action_3x3": (ou.fast_config(8, action={"type": "DiscreteAction"}), 27, 13, (5,)),
    "b15_linear_traffic": (ou.fast_config(8, other_vehicles_type=LINEAR), 15, 14, ()),
    "b15_lidar": (ou.fast_config(8, observation={"type": "LidarObservation", "cells": 16}), 15, 15, ()),
}
EVENTS = {
    "dense": (ou.fast_config(8, vehicles_density=3.0), 25, 1, ()),
    "short": (ou.fast_config(8, duration=2), 85, 2, ()),
    "lane0": (ou.fast_config(8, initial_lane_id=0), 15, 1, ()),
}
_cache = {}


def planned(backend: str, name: str):
    """(action, details, yardstick) of a case, computed once per backend."""
    key = (backend, name)
    if key not in _cache:
        config, budget, seed, warm = {**SHAPES, **EVENTS}[name]
        env = ou.make_env(backend, config, 3, seed, warm)
        action, details = env.plan_opd(budget, GAMMA, return_details=True)
        want = ou.restate_opd(backend, env, budget, GAMMA)
        env.close()
        _cache[key] = (action, details, want)
    return _cache[key]


@pytest.mark.parametrize("backend", ou.BACKENDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_plan_equals_the_restated_rules(backend, name):
    action, details, want = planned(backend, name)
    print(name, "action", action, "expanded", details["expanded"], "value", details["value"], "upper", details["upper"])
    assert action.dtype == np.int32 and action.shape == (3,)
    assert details["sequence"].shape == want["sequence"].shape and details["sequence"].dtype == np.int32
    ou.assert_plan_equals(action, details, want, name)


@pytest.mark.parametrize("backend", ou.BACKENDS)
@pytest.mark.parametrize("name", list(EVENTS))
def test_terminal_leaves_solved_trees_and_ties(backend, name):
    action, details, want = planned(backend, name)
    X = details["sequence"].shape[1]
    terminal = np.array([sum(nd["done"] for nd in tree) for tree in want["trees"]])
    print(name, "action", action, "expanded", details["expanded"], "terminal nodes", terminal, "tie", want["tie"], "value", details["value"],
          "upper", details["upper"])
    ou.assert_plan_equals(action, details, want, name)
    solved = details["expanded"] < X
    if name == "dense":
        crashed = [any(nd["done"] and (nd["state"]["st"]["flags"] & 1).any() for nd in tree) for tree in want["trees"]]
        assert any(crashed), "no crash among the nodes"
        # FASTER twice from the root: the episode is over within two steps somewhere
        assert any(tree[4]["done"] or (tree[4]["children"] is not None and tree[tree[4]["children"][3]]["done"]) for tree in want["trees"])
    if name == "short":
        assert X == 17 and solved.all() and (details["expanded"] == 6).all()
        ou.assert_bits(details["value"], details["upper"], "a solved tree's bounds meet")
        assert all(nd["done"] == (nd["disc"] < 0.6) for tree in want["trees"] for nd in tree[1:])   # exactly the depth-2 nodes
    if name == "lane0":
        assert want["tie"].any(), "no selection met two leaves of equal upper"
        tree = want["trees"][0]
        assert tree[1]["vup"] == tree[2]["vup"] and tree[1]["ret"] == tree[2]["ret"]   # LANE_LEFT == IDLE in lane 0
    assert (~solved | (details["value"] == details["upper"])).all()


@pytest.mark.parametrize("schedule", [dict(lane="desc"), dict(lane="seeded", seed=3)], ids=["lanes_descending", "lanes_seeded"])
def test_plan_does_not_depend_on_the_order_of_the_lanes(schedule):
    """The kernel under the emulator's other fiber orders (CPU only): the same plan, and no barrier met from two call sites."""
    name = "b85_second_lane_pass"
    config, budget, seed, warm = SHAPES[name]
    env = ou.make_env("emu", config, 3, seed, warm)
    env._engine.set_schedule(**schedule)
    action, details = env.plan_opd(budget, GAMMA, return_details=True)
    assert env._engine.schedule_errors() == 0, env._engine.schedule_error_text()
    env.close()
    ou.assert_plan_equals(action, details, planned("emu", name)[2], name)
