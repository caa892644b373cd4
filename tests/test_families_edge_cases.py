"""Edge cases of the Linear traffic family, of direct ego control (``DiscreteAction``) and of the ``LidarObservation`` against the
oracle: the degenerate and maximum sizes, the wavefront boundary, unusual frequencies and off-road termination of
tests/test_edge_cases.py, the Lidar kernel's own edges, and auto-reset.  Same comparison (tests/families_util.py: rollout), same
backends (``emu`` = the CPU emulation of the kernel source, ``hip`` = the MI355X)."""
import numpy as np
import pytest

from highwayenv_amd import _abi
from oracle import oracle
from tests.backends import BACKENDS
from tests.families_util import assert_lidar_of_own_state, comparable, compare_step, engine_state, make_engine, rollout

FAMILIES = ["linear", "direct", "lidar"]
LINEAR = {"other_vehicles_type": "highway_env.vehicle.behavior.LinearVehicle"}
DIRECT = {"action": {"type": "DiscreteAction", "steering_range": [-0.1, 0.1]}}
LIDAR = {"observation": {"type": "LidarObservation", "cells": 16, "maximum_range": 60}}


def family_config(family, fast=True, **over):
    """The family on highway-fast-v0 / highway-v0 defaults.  The Lidar family's dynamics alternate between the three step kernels
    it runs behind (`lidar`: IDM with meta-actions, `lidar-linear`, `lidar-direct`)."""
    cfg = _abi.highway_fast_default_config() if fast else _abi.highway_default_config()
    for part, upd in (("linear", LINEAR), ("direct", DIRECT), ("lidar", LIDAR)):
        if part in family:
            cfg.update(upd)
    cfg.update(over)
    return cfg


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("family", FAMILIES + ["lidar-direct"])
def test_ego_alone_on_the_road(backend, family):
    """No traffic: no neighbour, no obstacle to trace (every Lidar cell stays at the range)."""
    ref = rollout(backend, family_config(family, vehicles_count=0, lanes_count=2, duration=6), True, 3, 8, seed=1)
    assert ref["x"].shape == (3, 1)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("family", FAMILIES + ["lidar-linear"])
def test_single_lane(backend, family):
    ref = rollout(backend, family_config(family, vehicles_count=15, lanes_count=1), True, 4, 10, seed=2)
    assert (ref["lane"] == 0).all()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("family", FAMILIES + ["lidar-linear", "lidar-direct"])
@pytest.mark.parametrize("total", [63, 64, 65])
def test_wavefront_boundary(backend, family, total):
    """N = 63 / 64: the one-wavefront kernel with one / no idle lane; N = 65: the workgroup kernel with two wavefronts."""
    cfg = family_config(family, vehicles_count=total - 1, lanes_count=4)
    rollout(backend, cfg, True, 2 if backend == "emu" else 16, 3 if backend == "emu" else 8, seed=4 + total)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_maximum_sizes(backend, family):
    """N = 256 vehicles (4 wavefronts per environment) on 16 lanes, full pairwise collisions; the Lidar with its 64 cells."""
    cfg = family_config(family, fast=False, vehicles_count=255, lanes_count=16, simulation_frequency=5, duration=10)
    if family == "lidar":
        cfg["observation"] = dict(cfg["observation"], cells=64, maximum_range=150)
    rollout(backend, cfg, False, 1 if backend == "emu" else 4, 2 if backend == "emu" else 4, seed=3)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("family", FAMILIES + ["lidar-linear"])
def test_unusual_frequencies(backend, family):
    """simulation_frequency 12 with policy_frequency 4: three frames of 1/12 s per step, truncation after 12 steps."""
    cfg = family_config(family, fast=False, vehicles_count=20, lanes_count=3, simulation_frequency=12, policy_frequency=4, duration=3)
    ref = rollout(backend, cfg, False, 4, 14, seed=5)
    assert _abi.make_config(cfg, 1).frames_per_step == 3
    assert (ref["time"] == 14 * 0.25).all()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("family", ["direct", "lidar-direct"])
def test_offroad_termination_by_a_steered_ego(backend, family):
    """Steering held to the right (id 5 of the 3 x 3 table: no throttle, full right): the ego leaves the two-lane road, which
    terminates the episode (offroad_terminal) and zeroes the reward; no collision is involved."""
    cfg = family_config(family, vehicles_count=6, lanes_count=2, offroad_terminal=True, normalize_reward=False)
    cfg["action"] = {"type": "DiscreteAction", "steering_range": [-0.3, 0.3]}

    def clear_the_road(st):
        st["x"][:, 1:] += 500

    ref = rollout(backend, cfg, True, 4, 3, seed=6, mutate=clear_the_road, actions=[5])
    assert (ref["y"][:, 0] > 4.0 + 2.0).all() and not (ref["flags"] & _abi.F_CRASHED).any()
    assert (ref["ctl_steer"] == _abi.make_config(cfg, 1).steer_axis[2]).all()


# ---- the Lidar kernel's own edges ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("normalize", [False, True])
def test_lidar_range_smaller_than_every_gap(backend, normalize):
    """maximum_range 4 m on one lane, where no two centres come closer than a vehicle length: nothing is traced, the grid stays at
    the range (1.0 when normalised)."""
    cfg_d = family_config("lidar", vehicles_count=15, lanes_count=1,
                          observation={"type": "LidarObservation", "cells": 7, "maximum_range": 4.0, "normalize": normalize})
    cfg = _abi.make_config(cfg_d, 4, fast=True)
    eng = make_engine(backend, cfg)
    eng.reset(seeds=np.arange(4, dtype=np.uint64) + 9, ego_spacing=cfg_d["ego_spacing"], vehicles_density=cfg_d["vehicles_density"])
    want = np.float32(1.0 if normalize else 4.0)
    for t in range(3):
        obs = eng.step(np.ones((4, 1), np.int32))[0]
        assert_lidar_of_own_state(cfg, eng, obs, f"step {t}")
        st = eng.get_state()
        assert np.abs(np.diff(np.sort(st["x"], axis=1), axis=1)).min() > 4.0  # (what the case rests on)
        assert (obs == want).all()
    eng.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_lidar_64_cells_with_more_than_64_vehicles(backend):
    """64 cells and N = 81: one lane of the wavefront per cell, two obstacle passes of the kernel."""
    cfg = family_config("lidar", vehicles_count=80, lanes_count=4, vehicles_density=2.0,
                        observation={"type": "LidarObservation", "cells": 64, "maximum_range": 150, "normalize": False})
    rollout(backend, cfg, True, 2 if backend == "emu" else 8, 3 if backend == "emu" else 6, seed=8)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("family", ["lidar", "lidar-linear", "lidar-direct"])
def test_lidar_observers_that_are_not_vehicle_0(backend, family):
    """Three agents: the second and third observers sit in the middle of the vehicle list."""
    inner = {"type": "LidarObservation", "cells": 24, "maximum_range": 80}
    cfg = family_config(family, vehicles_count=20, lanes_count=3, controlled_vehicles=3,
                        observation={"type": "MultiAgentObservation", "observation_config": inner})
    act = cfg["action"]
    cfg["action"] = {"type": "MultiAgentAction", "action_config": act}
    assert list(_abi.make_config(cfg, 1, fast=True).agent_index[:3]) == [0, 8, 16]
    rollout(backend, cfg, True, 3, 6, seed=9)


@pytest.mark.parametrize("backend", BACKENDS)
def test_lidar_every_obstacle_pass_reaches_an_observer(backend):
    """N = 256 with three observers (vehicles 0, 86 and 171) and 64 cells: the obstacles around the second and third observer sit in
    the third and fourth pass of 64 (a single ego at the head of the list only ever sees the first)."""
    inner = {"type": "LidarObservation", "cells": 64, "maximum_range": 150, "normalize": False}
    cfg = family_config("lidar", vehicles_count=253, lanes_count=4, controlled_vehicles=3, vehicles_density=1.5,
                        observation={"type": "MultiAgentObservation", "observation_config": inner},
                        action={"type": "MultiAgentAction", "action_config": {"type": "DiscreteMetaAction"}})
    assert list(_abi.make_config(cfg, 1, fast=True).agent_index[:3]) == [0, 86, 171]
    rollout(backend, cfg, True, 1 if backend == "emu" else 4, 2 if backend == "emu" else 4, seed=10)


# ---- auto-reset ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("family", FAMILIES + ["lidar-linear", "lidar-direct"])
def test_autoreset_against_the_oracle(backend, family):
    """duration 3, Philox device re-spawn, 8 environments x 10 steps: every environment ends (at the latest) in its third step and
    is re-spawned in the next.  The oracle has no Philox: after every step it takes over the engine's state for the environments
    that step re-spawned (and checks what a re-spawn step returns: time 0, reward 0, not done); every other env-step is compared
    like in rollout() -- flags exact, reward 1e-9, state 1e-7, stored controls with the state, Lidar against the trace of the
    engine's own state -- up to an environment's first wreck.  Linear traffic: the re-spawned parameters are the rule's draws on
    the next episode's Philox stream (tests/test_traffic_parity.py: test_autoreset_respawns_parameters)."""
    E, STEPS, BASE = 8, 10, 1234
    cfg_d = family_config(family, vehicles_count=20, lanes_count=3, duration=3)
    cfg = _abi.make_config(cfg_d, E, fast=True)
    direct, linear = cfg.ego_control == _abi.EGO_DIRECT, cfg.traffic_model == _abi.TRAFFIC_LINEAR
    eng = make_engine(backend, cfg)
    spawn_args = dict(ego_spacing=cfg_d["ego_spacing"], vehicles_density=cfg_d["vehicles_density"])
    eng.reset(seeds=np.arange(E, dtype=np.uint64) + 50, **spawn_args)
    eng.set_autoreset(True, base_seed=BASE, **spawn_args)
    ref = engine_state(eng)
    rng = np.random.default_rng(17)
    done_prev, dead = np.zeros(E, bool), np.zeros(E, bool)
    episode = np.zeros(E, int)
    compared = respawns = 0
    for t in range(STEPS):
        acts = rng.integers(0, _abi.num_actions(cfg), size=(E, cfg.num_agents)).astype(np.int32)
        obs, reward, term, trunc, info = eng.step(acts)
        got = engine_state(eng)
        with oracle.impact_margins(cfg) as m:
            o2, r2, te2, tr2, _ = oracle.step(cfg, ref, acts)
        what = f"step {t}"
        # a re-spawn step: the new episode starts, nothing is rewarded, nothing ends
        assert (got["time"][done_prev] == 0.0).all() and not reward[done_prev].any(), what
        assert not term[done_prev].any() and not trunc[done_prev].any(), what
        episode += done_prev
        respawns += int(done_prev.sum())
        if linear:
            from tests.emu import emu
            for e in np.flatnonzero(done_prev):
                for i in range(1, cfg.num_vehicles):
                    np.testing.assert_array_equal(got["behavior"][e, i], emu.behavior_draw(BASE + e, i, int(episode[e])),
                                                  err_msg=f"{what}: env {e} vehicle {i}")
        if direct:  # Vehicle.__init__: the new ego's stored action is zero
            assert not got["ctl_accel"][done_prev].any() and not got["ctl_steer"][done_prev].any(), what
        dead &= ~done_prev
        live = ~done_prev & ~dead
        wreck, ok = comparable(ref, m.margin.min(1), live)
        # (a Lidar observation is checked on EVERY environment, re-spawn steps included: the new episode's first state)
        compare_step(cfg, eng, (obs, reward, term, trunc), ref, (o2, r2, te2, tr2), wreck, ok, live, what, trunc_rows=live)
        compared += int(ok.sum())
        dead |= live & wreck
        take = done_prev | dead  # the oracle follows the engine through re-spawns, and through wrecks until their re-spawn
        for k in ref:
            ref[k][take] = got[k][take]
        done_prev = np.asarray(term | trunc, bool)
    eng.close()
    assert respawns >= 2 * E and compared >= 0.5 * E * STEPS, (respawns, compared)
