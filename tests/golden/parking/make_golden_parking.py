#!/usr/bin/env python3
"""Generate the parking fixtures in this directory from the UNMODIFIED reference (``ParkingEnv``, envs/parking_env.py).

TEST INFRASTRUCTURE.  Needs the reference package (``HWY_REFERENCE_ROOT``), imported through ``oracle/ref_stub.py`` by way of
tests/golden/control/make_golden_control.py like the other generators:

    python tests/golden/parking/make_golden_parking.py [fixture ...]

Every fixture but ``reset_rule`` is ONE environment stepped with recorded float32 actions.  Arrays (T policy steps, n parked vehicles):
  ``config_json``                         the config the env was built with
  ``init_ego``  f64 [4]                   x, y, heading, speed before the first step (after any placement through the reference's own
                                          attributes: ``vehicle.position`` / ``heading`` / ``speed``)
  ``goal``, ``order`` [n]                 spot of the goal Landmark and of every parked vehicle, in Road.vehicles order
  ``actions``  f32 [T, 2]
  ``ego``      f64 [T, 8]                 x, y, heading, speed, stored acceleration, stored steering, impact_x, impact_y after the step
  ``ego_crashed``, ``ego_has_impact`` [T]
  ``parked``   f64 [T, n, 4]              x, y, heading, speed;  ``parked_crashed`` [T, n]
  ``obs``      f64 [T, 3, 6]              observation, achieved_goal, desired_goal
  ``reward`` f64 [T], ``terminated`` / ``truncated`` / ``is_success`` [T]
  ``first_crash_step``                    -1 or the step of the ego's first crash, which is the LAST recorded step (terminated); ``margin`` the smallest distance, up to the frame of
                                          the ego's first verdict, of a pre-check from its sphere and of a SAT interval from zero
``reset_rule.npz``: for 256 seeds of a 26-vehicle lot the heading, the ego's spot, the goal's spot and the parked spots.
Crash and success cases are asserted decisive here: margins above 1e-6.  Digests go to MANIFEST.json.
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location("make_golden_control", os.path.join(GOLDEN, "control", "make_golden_control.py"))
control = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(control)  # (installs oracle/ref_stub.py's stand-ins and imports the reference)

from highway_env import utils  # noqa: E402
from highway_env.envs.parking_env import ParkingEnv  # noqa: E402
from highway_env.vehicle.objects import RoadObject  # noqa: E402

MARGIN = {"value": np.inf, "ego": None, "solid": False}


def _watching() -> bool:
    """Up to and including the FRAME of the ego's first verdict: a body pushed back by its impact then rests AT the other's face,
    and touching is not a decision to hold."""
    ego = MARGIN["ego"]
    return MARGIN["solid"] and ego is not None and not ego.crashed and ego.impact is None
_interval_distance, _is_colliding = utils.interval_distance, RoadObject._is_colliding


def _watched_interval_distance(*a):
    d = _interval_distance(*a)
    if _watching():
        MARGIN["value"] = min(MARGIN["value"], abs(d))
    return d


def _watched_is_colliding(self, other, dt):
    # the ego's pairs with solid bodies (the goal Landmark is not solid: a pair with it decides nothing observable; up to the ego's
    # first verdict every other pair is a RESTING pair, separated by metres on a SAT axis whatever its pre-check says -- the vehicle
    # on (-14, -14) and the wall at y = 21 sit exactly ON each other's sphere: 14^2 + 35^2 = 1421, (sqrt(29) + sqrt(4901)) / 2)
    MARGIN["solid"] = self is MARGIN["ego"] and self.solid and other.solid
    if _watching():
        gap = np.linalg.norm(other.position - self.position) - ((self.diagonal + other.diagonal) / 2 + self.speed * dt)
        MARGIN["value"] = min(MARGIN["value"], abs(gap))
    return _is_colliding(self, other, dt)


utils.interval_distance = _watched_interval_distance
RoadObject._is_colliding = _watched_is_colliding


def spot_of(lane_index) -> int:
    return (0 if lane_index[0] == "a" else 14) + lane_index[2]


def spot_at(position) -> int:
    return (0 if position[1] > 0 else 14) + int(round((position[0] + 26.0) / 4.0))


FULL = np.array([1.0, 0.0], np.float32)
CASES = [
    # default lot, random float32 actions beyond +-1 (np.clip works; negative throttle: reverse driving), run to truncation (step 101: a
    # hundred additions of 1 / 5 stay below 20); main() moves on to the next action stream until one stays clear of the walls
    dict(name="free_0", config={"duration": 20}, seed=0, steps=101, action_seed=11, no_crash=True),
    dict(name="free_1", config={"duration": 20}, seed=1, steps=101, action_seed=12, no_crash=True),
    dict(name="free_2", config={"duration": 20}, seed=2, steps=101, action_seed=13, no_crash=True),
    # full throttle into the long wall (y = 21) and the short wall (x = 35)
    dict(name="wall_long", config={"duration": 20}, seed=3, steps=30, heading=1.3, action=FULL, crash=True),
    dict(name="wall_short", config={"duration": 20}, seed=4, steps=30, heading=0.2, action=FULL, crash=True),
    # into a parked vehicle (aimed at parked vehicle 0, slightly off centre); every spot taken
    dict(name="parked_10", config={"duration": 20, "vehicles_count": 10}, seed=5, steps=25, aim=0.06, action=FULL, crash=True),
    dict(name="parked_26", config={"duration": 20, "vehicles_count": 26}, seed=6, steps=25, aim=-0.04, action=FULL, crash=True),
    dict(name="parked_10_free", config={"duration": 20, "vehicles_count": 10}, seed=7, steps=101, action_seed=14, no_crash=True),
    # no walls: the ego leaves the lot and nothing happens
    dict(name="no_walls", config={"duration": 20, "add_walls": False}, seed=8, steps=60, heading=0.3, action=FULL),
    # parking-ActionRepeat-v0: 15 frames per policy step
    dict(name="repeat", config={"policy_frequency": 1, "duration": 20}, seed=9, steps=20, action_seed=15),
    # next to the goal: is_success and terminated without a crash; and just outside success_goal_reward
    dict(name="success_in", config={"duration": 20}, seed=10, steps=3, near=(0.3, 0.2, 0.05), action=np.zeros(2, np.float32), success=True),
    dict(name="success_out", config={"duration": 20}, seed=10, steps=3, near=(1.5, 0.0, 0.0), action=np.zeros(2, np.float32), success=False),
]


def record(case) -> dict:
    env = ParkingEnv(case["config"])
    env.reset(seed=case["seed"])
    ego, parked = env.road.vehicles[0], env.road.vehicles[1:]
    if "heading" in case:
        ego.heading = case["heading"]
    if "aim" in case:
        ego.heading = float(np.arctan2(parked[0].position[1], parked[0].position[0])) + case["aim"]
    if "near" in case:
        dx, dy, dh = case["near"]
        ego.position = ego.goal.position + np.array([dx, dy])
        ego.heading = float(ego.goal.heading + dh)
    T, n = case["steps"], len(parked)
    rng = np.random.default_rng(case.get("action_seed", 0))
    out = {"config_json": np.array(json.dumps(case["config"])), "init_ego": np.array([*ego.position, ego.heading, ego.speed]),
           "goal": np.int32(spot_at(ego.goal.position)), "order": np.array([spot_at(v.position) for v in parked], np.int32),
           "actions": np.zeros((T, 2), np.float32), "ego": np.zeros((T, 8)), "ego_crashed": np.zeros(T, bool),
           "ego_has_impact": np.zeros(T, bool), "parked": np.zeros((T, n, 4)), "parked_crashed": np.zeros((T, n), bool),
           "obs": np.zeros((T, 3, 6)), "reward": np.zeros(T), "terminated": np.zeros(T, bool), "truncated": np.zeros(T, bool),
           "is_success": np.zeros(T, bool)}
    MARGIN.update(value=np.inf, ego=ego)
    first_crash = -1
    for t in range(T):
        a = case["action"] if "action" in case else rng.uniform(-1.3, 1.3, 2).astype(np.float32)
        obs, reward, term, trunc, info = env.step(a)
        imp = ego.impact if ego.impact is not None else np.zeros(2)
        out["actions"][t] = a
        out["ego"][t] = [*ego.position, ego.heading, ego.speed, ego.action["acceleration"], ego.action["steering"], *imp]
        out["ego_crashed"][t], out["ego_has_impact"][t] = ego.crashed, ego.impact is not None
        for i, v in enumerate(parked):
            out["parked"][t, i] = [*v.position, v.heading, v.speed]
            out["parked_crashed"][t, i] = v.crashed
        out["obs"][t] = [obs["observation"], obs["achieved_goal"], obs["desired_goal"]]
        out["reward"][t], out["terminated"][t], out["truncated"][t], out["is_success"][t] = reward, term, trunc, info["is_success"]
        if ego.crashed and first_crash < 0:
            first_crash = t
    out["first_crash_step"], out["margin"] = np.int32(first_crash), np.float64(MARGIN["value"])
    goal_reward = out["reward"] - env.config["collision_reward"] * out["ego_crashed"]
    out["success_margin"] = np.float64(np.abs(goal_reward + env.config["success_goal_reward"]).min())
    if case.get("crash"):
        assert first_crash >= 0, case["name"]
    if case.get("crash") or "success" in case:
        assert out["margin"] > 1e-6 and out["success_margin"] > 1e-6, (case["name"], out["margin"], out["success_margin"])
    if "success" in case:
        assert first_crash < 0 and bool(out["is_success"][0]) is case["success"] and bool(out["terminated"][0]) is case["success"]
    if first_crash >= 0:  # the episode is over (terminated): a body pushed back by its impact then rests AT the other's face, and
        T = first_crash + 1  # every later frame decides `distance > 0` on a distance of 1e-15 -- nothing the reference itself holds
        out = {k: (v[:T] if isinstance(v, np.ndarray) and v.ndim and k not in ("init_ego", "order") else v) for k, v in out.items()}
    print(f"{case['name']:16s} T={T:3d} parked={n:2d} first_crash={first_crash:3d} margin={out['margin']:.3g} "
          f"success={int(out['is_success'].sum())} truncated={int(out['truncated'].sum())} speed in [{out['ego'][:, 3].min():.2f}, {out['ego'][:, 3].max():.2f}] "
          f"parked_crashed={int(out['parked_crashed'][-1].sum())}")
    return out


def reset_rule(n_seeds=256) -> dict:
    out = {"heading": np.zeros(n_seeds), "ego_spot": np.zeros(n_seeds, np.int32), "goal": np.zeros(n_seeds, np.int32),
           "order": np.zeros((n_seeds, 26), np.int32)}
    env = ParkingEnv({"vehicles_count": 26})
    for s in range(n_seeds):
        env.reset(seed=s)
        ego = env.road.vehicles[0]
        out["heading"][s], out["ego_spot"][s], out["goal"][s] = ego.heading, spot_of(ego.lane_index), spot_at(ego.goal.position)
        out["order"][s] = [spot_at(v.position) for v in env.road.vehicles[1:]]
    print("reset_rule: ego spots", sorted(set(out["ego_spot"].tolist())))
    return out


def main(argv):
    manifest_path = os.path.join(HERE, "MANIFEST.json")
    manifest = json.load(open(manifest_path)) if os.path.exists(manifest_path) else {}
    todo = [c for c in CASES if not argv or c["name"] in argv]
    results = {}
    for c in todo:
        results[c["name"]] = record(c)
        while c.get("no_crash") and results[c["name"]]["first_crash_step"] >= 0:  # the next action stream that stays clear
            c["action_seed"] += 100
            results[c["name"]] = record(c)
        if c.get("no_crash"):
            print(f"  {c['name']}: action_seed {c['action_seed']}")
    if not argv or "reset_rule" in argv:
        results["reset_rule"] = reset_rule()
    for name, arrays in results.items():
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **arrays)
        manifest[name] = control.digest(arrays)
    json.dump(manifest, open(manifest_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main(sys.argv[1:])
