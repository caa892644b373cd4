"""The device-side fork is the existing host route: after ``fork_from`` the child's state, behaviour parameters and stored controls
are ``np.repeat`` of the parent's, a K = 3 rollout of the child equals, bit for bit, the same rollout of an engine filled through
``get_state`` / ``set_state`` (+ ``set_behavior`` / ``set_controls``), the parent is left exactly as it was, and a ``fork(1)`` child
stepped in lock step with its parent gives identical outputs.  States are compared through ``get_state`` (``set_state`` need not
keep the rank hint of the packed word, and no result depends on it).

Shapes: E = 3; N = 8, 21, 65, 130 (pitch 8 / 24 / 72 / 136, all three step kernels); Linear traffic, a DiscreteAction ego and two
agents at N = 21; ``source`` with repeated, out-of-order and omitted parents.  Runs on the CPU emulation of the kernel source and,
marked ``gpu``, on the MI355X."""
import numpy as np
import pytest

from highwayenv_amd import _abi
from tests import lookahead_util as lu

E = 3
LINEAR = "highway_env.vehicle.behavior.LinearVehicle"
MA = {"controlled_vehicles": 2, "action": {"type": "MultiAgentAction", "action_config": {"type": "DiscreteMetaAction"}},
      "observation": {"type": "MultiAgentObservation", "observation_config": {"type": "Kinematics"}}}
CASES = {
    "n8": (lu.highway_config(8), 3), "n21": (lu.highway_config(21), 25), "n65": (lu.highway_config(65), 2), "n130": (lu.highway_config(130), 2),
    "linear21": (lu.highway_config(21, other_vehicles_type=LINEAR), 3),
    "direct21": (lu.highway_config(21, action={"type": "DiscreteAction", "steering_range": [-0.1, 0.1]}), 3),
    "ma21": (lu.highway_config(21, **MA), 3),
    "grid21": (lu.highway_config(21, observation={"type": "OccupancyGrid"}), 2),
    "lidar21": (lu.highway_config(21, observation={"type": "LidarObservation", "cells": 16}), 2),
}


def _parent(backend, config, steps=2, seed=7):
    cfg = _abi.make_config(config, E, fast=True)
    eng = lu.make_engine(backend, cfg)
    eng.set_autoreset(False)
    eng.reset(seeds=np.arange(E, dtype=np.uint64) + np.uint64(seed))
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        eng.step(rng.integers(0, _abi.num_actions(cfg), size=(E, cfg.num_agents)).astype(np.int32))
    return cfg, eng


def _extras(eng):
    out = {}
    if eng.cfg.traffic_model == _abi.TRAFFIC_LINEAR:
        out["behavior"] = eng.get_behavior()
    if eng.cfg.ego_control == _abi.EGO_DIRECT:
        out["acceleration"], out["steering"] = eng.get_controls()
    return out


def _filled_by_the_host_route(backend, cfg, parent, index):
    """The route that existed before: get_state -> np.repeat -> set_state (+ set_behavior / set_controls)."""
    eng = lu.make_engine(backend, lu.with_envs(cfg, len(index)))
    eng.set_autoreset(False)
    eng.set_state(lu.repeat_state(parent.get_state(), index))
    ex = _extras(parent)
    if "behavior" in ex:
        eng.set_behavior(np.ascontiguousarray(ex["behavior"][index]))
    if "acceleration" in ex:
        eng.set_controls(np.ascontiguousarray(ex["acceleration"][index]), np.ascontiguousarray(ex["steering"][index]))
    return eng


def _assert_outputs_equal(a, b, what):
    for x, y, k in zip(a[:4], b[:4], ("obs", "reward", "terminated", "truncated")):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {k}")
    lu.assert_bits(a[1], b[1], f"{what}: reward bits")
    for k in ("speed", "crashed"):
        np.testing.assert_array_equal(a[4][k], b[4][k], err_msg=f"{what}: info {k}")


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("backend", lu.BACKENDS)
def test_fork_is_the_host_route(backend, case):
    config, B = CASES[case]
    cfg, parent = _parent(backend, config)
    before, extras_before = parent.get_state(), _extras(parent)
    index = np.arange(E * B) // B
    child = lu.make_engine(backend, lu.with_envs(cfg, E * B))
    child.set_autoreset(False)
    child.fork_from(parent, B)
    lu.assert_states_equal(child.get_state(), lu.repeat_state(before, index), f"{case}: the child's state")
    for k, v in _extras(child).items():
        lu.assert_bits(v, np.ascontiguousarray(extras_before[k][index]), f"{case}: the child's {k}")
    host = _filled_by_the_host_route(backend, cfg, parent, index)
    acts = np.random.default_rng(11).integers(0, _abi.num_actions(cfg), size=(3, E * B, cfg.num_agents)).astype(np.int32)
    _assert_outputs_equal(child.rollout(acts), host.rollout(acts), f"{case}: K = 3 rollout")
    lu.assert_states_equal(child.get_state(), host.get_state(), f"{case}: the state after the rollout")
    lu.assert_states_equal(parent.get_state(), before, f"{case}: the parent")
    for k, v in _extras(parent).items():
        lu.assert_bits(v, extras_before[k], f"{case}: the parent's {k}")
    for eng in (parent, child, host):
        eng.close()


@pytest.mark.parametrize("case", ["n21", "linear21", "direct21", "n65"])
@pytest.mark.parametrize("backend", lu.BACKENDS)
def test_fork_with_source_indices(backend, case):
    """Repeated, out-of-order and omitted parents; a child that is not a multiple of the parent."""
    config, _ = CASES[case]
    cfg, parent = _parent(backend, config)
    source = np.array([2, 0, 2, 2, 0], np.int32)   # parent 1 is omitted
    child = lu.make_engine(backend, lu.with_envs(cfg, len(source)))
    child.set_autoreset(False)
    child.fork_from(parent, 1, source)
    lu.assert_states_equal(child.get_state(), lu.repeat_state(parent.get_state(), source), case)
    for k, v in _extras(child).items():
        lu.assert_bits(v, np.ascontiguousarray(_extras(parent)[k][source]), f"{case}: {k}")
    host = _filled_by_the_host_route(backend, cfg, parent, source)
    acts = np.random.default_rng(12).integers(0, _abi.num_actions(cfg), size=(3, len(source), cfg.num_agents)).astype(np.int32)
    _assert_outputs_equal(child.rollout(acts), host.rollout(acts), f"{case}: K = 3 rollout")
    for eng in (parent, child, host):
        eng.close()


@pytest.mark.parametrize("case", ["n21", "n130", "ma21"])
@pytest.mark.parametrize("backend", lu.BACKENDS)
def test_fork_1_steps_in_lock_step_with_its_parent(backend, case):
    config, _ = CASES[case]
    cfg, parent = _parent(backend, config)
    child = lu.make_engine(backend, lu.with_envs(cfg, E))
    child.set_autoreset(False)
    child.fork_from(parent, 1)
    rng = np.random.default_rng(13)
    for t in range(5):
        a = rng.integers(0, _abi.num_actions(cfg), size=(E, cfg.num_agents)).astype(np.int32)
        _assert_outputs_equal(parent.step(a), child.step(a), f"{case}: step {t}")
    lu.assert_states_equal(parent.get_state(), child.get_state(), case)
    parent.close(), child.close()


@pytest.mark.parametrize("backend", lu.BACKENDS)
def test_a_finished_parent_is_forked_as_it_stands(backend):
    """An environment that awaits its NextStep re-spawn: the child continues the ended episode (its `done` mark is cleared), the
    parent re-spawns at its next step."""
    config = lu.highway_config(21, duration=2)
    cfg = _abi.make_config(config, E, fast=True)
    parent = lu.make_engine(backend, cfg)
    parent.reset(seeds=np.arange(E, dtype=np.uint64))
    parent.set_autoreset(True, base_seed=99)
    idle = np.ones((E, 1), np.int32)
    for _ in range(2):
        out = parent.step(idle)
    assert out[3].all()   # truncated: every environment awaits its re-spawn
    child = lu.make_engine(backend, lu.with_envs(cfg, E))
    child.set_autoreset(False)
    child.fork_from(parent, 1)
    lu.assert_states_equal(child.get_state(), parent.get_state(), "the child of a finished parent")
    c = child.step(idle)
    assert c[3].all() and (child.get_state()["time"] == 3.0).all()   # the ended episode goes on
    p = parent.step(idle)
    assert not p[3].any() and (parent.get_state()["time"] == 0.0).all()   # the parent was re-spawned instead
    parent.close(), child.close()


@pytest.mark.parametrize("backend", lu.BACKENDS)
def test_env_fork_and_the_twin_that_never_planned(backend):
    """BatchedHighwayEnv.fork / score_sequences / plan_lookahead leave the parent as it was: its next step equals that of a twin
    that never planned; the child is cached per (num_envs, branches); `source` picks parents."""
    cls = lu.env_class(backend)
    config = lu.highway_config(21)
    env, twin = cls(config, num_envs=E, spawn_mode="device"), cls(config, num_envs=E, spawn_mode="device")
    env.reset(seed=5), twin.reset(seed=5)
    a = np.array([0, 3, 2])
    _assert_env_steps_equal(env.step(a), twin.step(a))
    before = env.get_state()
    best = env.plan_lookahead(2, horizon=3, gamma=0.9)
    assert best.shape == (E,) and best.dtype == np.int32 and ((best >= 0) & (best < 5)).all()
    returns, details = env.score_sequences(np.array([[1, 1], [0, 4], [3, 3]]), return_details=True)
    assert returns.shape == (E, 3) and details["reward"].shape == (E, 3, 2) and details["q"].shape == (E, 5)
    assert np.isneginf(details["q"][:, 2]).all() and np.isneginf(details["q"][:, 4]).all()   # no sequence starts with 2 or 4
    lu.assert_states_equal(env.get_state(), before, "the parent after planning")
    _assert_env_steps_equal(env.step(best), twin.step(best))
    child = env.fork(2)
    assert child.num_envs == 2 * E and env.fork(2) is child and not child.autoreset
    lu.assert_states_equal(child.get_state(), lu.repeat_state(env.get_state(), np.arange(2 * E) // 2), "fork(2)")
    picked = env.fork(1, source=[2, 2, 0, 1])
    lu.assert_states_equal(picked.get_state(), lu.repeat_state(env.get_state(), np.array([2, 2, 0, 1])), "fork(source)")
    obs, reward, term, trunc, info = child.step(np.ones(2 * E, np.int64))   # the child is an environment of its own
    assert obs.shape[0] == 2 * E and reward.shape == (2 * E,)
    env.close(), twin.close()


def _assert_env_steps_equal(a, b):
    for x, y in zip(a[:4], b[:4]):
        np.testing.assert_array_equal(x, y)
