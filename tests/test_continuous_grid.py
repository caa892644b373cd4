"""Two yardsticks for the whole continuous step that are independent of the fixtures.

Grid equivalence: in the reference ``DiscreteAction.act(i)`` IS ``ContinuousAction.act(all_actions[i])`` (action.py:189-196), so a
continuous run on actions that are exactly ``np.linspace(-1, 1, k, dtype=float32)`` grid points equals the ``DiscreteAction`` run
with ``actions_per_axis = k`` on the same seeds and ranges -- everything bit for bit: observations, rewards, flags, info, the final
state and the stored controls, through next-step auto-resets and through the device SameStep sequence.

Oracle: with the restated pair (tests/continuous_util.py) put into the C oracle's stored controls, ``oracle.frames`` with no ids
reproduces the engine's state after ``step_continuous`` at the suite's per-frame tolerance, for actions on no grid."""
import numpy as np
import pytest

from highwayenv_amd import _abi
from oracle import oracle
from tests.continuous_util import BACKENDS, assert_states_equal, make_engine, params_of, restate

F32 = np.float32
RANGES = {"acceleration_range": [-3.3, 2.1], "steering_range": [-0.07, 0.05]}
OBS = {"Kinematics": {"type": "Kinematics"}, "Lidar": {"type": "LidarObservation", "cells": 16}, "OccupancyGrid": {"type": "OccupancyGrid"}}


def _config(k, obs="Kinematics", n=20, agents=1, fast=True, duration=3, **act):
    d = _abi.highway_fast_default_config() if fast else _abi.highway_default_config()
    action = dict({"type": "DiscreteAction", "actions_per_axis": k}, **RANGES, **act)
    d.update({"vehicles_count": n, "lanes_count": 3, "duration": duration, "controlled_vehicles": agents,
              "observation": OBS[obs] if agents == 1 else {"type": "MultiAgentObservation", "observation_config": OBS[obs]},
              "action": action if agents == 1 else {"type": "MultiAgentAction", "action_config": action}})
    return d


def _grid_points(cfg, params, ids, k):
    """The float32 grid points of DiscreteAction ids [..]: (axis[id // n_steer], axis[id % n_steer]) -> [.., size]."""
    axis = np.linspace(-1, 1, k, dtype=F32)
    ids = np.asarray(ids)
    comps = ([axis[ids // cfg.n_steer]] if params.longitudinal else []) + ([axis[ids % cfg.n_steer]] if params.lateral else [])
    return np.stack(comps, -1).astype(F32)


def _pair(backend, d, E, fast=True, tuning=None, seed0=7):
    cfg = _abi.make_config(d, E, fast=fast, tuning=tuning)
    engines = [make_engine(backend, cfg) for _ in range(2)]
    kw = dict(ego_spacing=d["ego_spacing"], vehicles_density=d["vehicles_density"])
    first = [eng.reset(seeds=np.arange(E, dtype=np.uint64) + seed0, **kw) for eng in engines]
    np.testing.assert_array_equal(first[0], first[1])
    for eng in engines:
        eng.set_autoreset(True, base_seed=1000 + seed0, **kw)
    return cfg, engines


CASES = [pytest.param(3, "Kinematics", 20, 1, {}, id="k3-kinematics"), pytest.param(5, "Kinematics", 50, 1, {}, id="k5-kinematics-n50"),
         pytest.param(3, "Lidar", 20, 1, {}, id="k3-lidar"), pytest.param(5, "OccupancyGrid", 20, 1, {}, id="k5-grid"),
         pytest.param(5, "Kinematics", 100, 1, {}, id="k5-n100-workgroup"), pytest.param(3, "Kinematics", 20, 2, {}, id="k3-two-agents"),
         pytest.param(5, "Kinematics", 20, 1, {"lateral": False}, id="k5-longitudinal-only"),
         pytest.param(3, "Kinematics", 20, 1, {"longitudinal": False}, id="k3-lateral-only")]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("k,obs,n,agents,act", CASES)
def test_grid_points_equal_the_discrete_action_run(backend, k, obs, n, agents, act):
    """8 steps with episodes of 3 (every environment ends and is re-spawned by the next-step auto-reset inside the run): ids on one
    engine, their grid points on the other.  In the step that re-spawns an environment its stored controls are zero on both."""
    E = 64
    d = _config(k, obs, n, agents, **act)
    cfg, (disc, cont) = _pair(backend, d, E)
    params = params_of(d["action"])
    rng = np.random.default_rng(100 * k + n)
    done_prev = np.zeros(E, bool)
    respawns = 0
    for t in range(8):
        ids = rng.integers(0, _abi.num_actions(cfg), size=(E, agents)).astype(np.int32)
        a = disc.step(ids)
        b = cont.step_continuous(params, _grid_points(cfg, params, ids, k))
        for j in range(4):
            np.testing.assert_array_equal(a[j], b[j], err_msg=f"step {t} output {j}")
        for key in ("speed", "crashed"):
            np.testing.assert_array_equal(a[4][key], b[4][key], err_msg=f"step {t} info {key}")
        ca, cb = disc.get_controls(), cont.get_controls()
        for x, y in zip(ca, cb):
            np.testing.assert_array_equal(x.view(np.uint64), y.view(np.uint64), err_msg=f"step {t}: stored controls")
        if done_prev.any():  # re-spawned in this step: Vehicle.__init__'s zero action, whatever the act launch wrote before
            assert not cb[0][done_prev].any() and not cb[1][done_prev].any()
            respawns += int(done_prev.sum())
        done_prev = a[2] | a[3]
    assert respawns >= E
    assert_states_equal(disc.get_state(), cont.get_state())
    disc.close()
    cont.close()


@pytest.mark.parametrize("k,obs,agents", [(3, "Kinematics", 1), (5, "OccupancyGrid", 1), (3, "Lidar", 2)])
def test_grid_points_equal_the_discrete_run_through_the_same_step_sequence(k, obs, agents):
    """hwy_step_same_step_continuous_device's sequence on the emulation (act, step, stash, re-spawn) against
    hwy_step_same_step_device's on ids: every plane bit for bit, the ``final_obs`` rows and the mask included (the rows of
    environments that did not end keep their sentinel on both).  The engine's form: tests/test_continuous_vector.py."""
    E = 64
    d = _config(k, obs, 20, agents)
    cfg, (disc, cont) = _pair("emu", d, E)
    params = params_of(d["action"])
    rng = np.random.default_rng(k)
    ended = 0
    for t in range(7):
        ids = rng.integers(0, _abi.num_actions(cfg), size=(E, agents)).astype(np.int32)
        a = disc.step_same_step(ids)
        b = cont.step_same_step_continuous(params, _grid_points(cfg, params, ids, k))
        assert set(a) == set(b)
        for key in a:
            x, y = a[key], b[key]
            np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), err_msg=f"step {t}: {key}")
        ended += int(a["final_mask"].sum())
        for x, y in zip(disc.get_controls(), cont.get_controls()):
            np.testing.assert_array_equal(x, y)
        assert not cont.get_controls()[0][a["final_mask"] == 1].any()  # re-spawned in the same call: zero controls
    assert ended >= E
    assert_states_equal(disc.get_state(), cont.get_state())


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n,fast,agents", [(20, True, 1), (50, True, 2), (100, False, 1)])
def test_oracle_frames_on_the_restated_pair(backend, n, fast, agents):
    """Random actions on no grid, beyond the clip too.  Before every step the engine's state goes to the C oracle with the
    RESTATED pair as its stored controls; ``oracle.frames(cfg, st, None, T)`` then matches the engine's state after
    ``step_continuous`` at 1e-9 (the per-frame tolerance of tests/test_control_parity.py and tests/test_fuzz_configs.py), lanes and
    flags exact, the egos' speed and the stored controls bit for bit (exactly rounded recurrences)."""
    E, steps = 64, 3 if n == 100 else 6
    d = _config(3, "Kinematics", n, agents, fast=fast, duration=40)
    cfg = _abi.make_config(d, E, fast=fast)
    params = params_of(d["action"])
    eng = make_engine(backend, cfg)
    eng.reset(seeds=np.arange(E, dtype=np.uint64) + 31, ego_spacing=d["ego_spacing"], vehicles_density=d["vehicles_density"])
    rng = np.random.default_rng(n)
    agents_idx = list(cfg.agent_index[:agents])
    for t in range(steps):
        acts = rng.uniform(-1.3, 1.3, size=(E, agents, params.size)).astype(F32)
        st = eng.get_state()
        st["ctl_accel"], st["ctl_steer"] = (np.ascontiguousarray(p) for p in restate(params, acts))
        eng.step_continuous(params, acts)
        oracle.frames(cfg, st, None, cfg.frames_per_step)
        got = eng.get_state()
        for key in ("lane", "target_lane", "flags"):
            np.testing.assert_array_equal(got[key], st[key], err_msg=f"step {t}: {key}")
        for key in ("x", "y", "heading", "speed"):
            np.testing.assert_allclose(got[key], st[key], rtol=0, atol=1e-9, err_msg=f"step {t}: {key}")
        np.testing.assert_array_equal(got["speed"][:, agents_idx], st["speed"][:, agents_idx], err_msg=f"step {t}: the egos' speed")
        accel, steer = eng.get_controls()
        np.testing.assert_array_equal(accel, st["ctl_accel"], err_msg=f"step {t}: stored acceleration")
        np.testing.assert_array_equal(steer, st["ctl_steer"], err_msg=f"step {t}: stored steering")
    eng.close()
