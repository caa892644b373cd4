#!/usr/bin/env python3
"""Generate the direct-ego-control (``DiscreteAction``) fixtures in this directory from the UNMODIFIED reference.

TEST INFRASTRUCTURE.  Needs the reference package (``HWY_REFERENCE_ROOT``), imported through ``oracle/ref_stub.py`` like the
other generators:

    python tests/golden/control/make_golden_control.py [fixture ...]

Each fixture records a ``HighwayEnv`` / ``HighwayEnvFast`` run whose ``config["action"]`` is a ``DiscreteAction`` (or a
``MultiAgentAction`` over one): the initial state, the state after every frame for the first ``frames_for`` environments, the
state and obs / reward / terminated / truncated after every step.  The ego is a plain ``Vehicle``: its recorded
``target_speed`` is 0.0 (what ``getattr(ego, "target_speed", 0)`` yields, behavior.py:172), its ``target_lane`` is its lane,
its ``speed_index`` -1.  ``act_accel`` / ``act_steering`` hold every vehicle's stored action AFTER ``clip_actions`` wrote into
it (the agents' entries are the stored controls of the engine), ``all_actions`` the table ``DiscreteAction.act`` built (float32)
and ``axis_accel`` / ``axis_steer`` the physical values ``get_action`` mapped the axes to.  README.md states the one
assumption about gymnasium the table rests on.  The digests of the arrays go to ``MANIFEST.json`` here.
"""
from __future__ import annotations

import hashlib
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
sys.path.insert(0, ROOT)

from oracle import ref_stub  # noqa: E402

ref_stub.install()


class ArrayBox(ref_stub._Box):
    """``gymnasium.spaces.Box`` keeps ``low`` / ``high`` as ARRAYS of the space's shape and dtype
    (``np.full(shape, value, dtype)``); the stub of oracle/ref_stub.py keeps the scalars it was given, on which
    ``DiscreteAction.act`` (``np.linspace(low, high, k).T`` then ``itertools.product(*axes)``) fails."""

    def __init__(self, low=None, high=None, shape=None, dtype=np.float32, seed=None):
        super().__init__(low, high, shape, dtype, seed)
        if self.shape is not None:
            self.low = np.full(self.shape, low, dtype=self.dtype) if np.ndim(low) == 0 else np.asarray(low, self.dtype)
            self.high = np.full(self.shape, high, dtype=self.dtype) if np.ndim(high) == 0 else np.asarray(high, self.dtype)


sys.modules["gymnasium.spaces"].Box = ArrayBox

from highway_env.envs.highway_env import HighwayEnv, HighwayEnvFast  # noqa: E402
from highway_env.vehicle.behavior import IDMVehicle  # noqa: E402

F64_FIELDS = ["x", "y", "heading", "speed", "timer", "target_speed", "delta", "impact_x", "impact_y", "act_steering", "act_accel"]
I8_FIELDS = ["lane", "target_lane", "speed_index", "crashed", "has_impact", "check_collisions", "controlled"]


def dump_state(env) -> dict:
    """tests/golden/make_golden.py's record for a road whose controlled vehicles are plain Vehicles."""
    vs = env.road.vehicles
    n = len(vs)
    out = {k: np.zeros(n, np.float64) for k in F64_FIELDS}
    out.update({k: np.zeros(n, np.int8) for k in I8_FIELDS})
    for i, v in enumerate(vs):
        out["x"][i], out["y"][i] = v.position
        out["heading"][i] = v.heading
        out["speed"][i] = v.speed
        out["timer"][i] = getattr(v, "timer", np.nan)
        out["target_speed"][i] = getattr(v, "target_speed", 0)
        out["delta"][i] = v.DELTA if isinstance(v, IDMVehicle) else np.nan
        if v.impact is not None:
            out["impact_x"][i], out["impact_y"][i] = v.impact
            out["has_impact"][i] = 1
        out["act_steering"][i] = v.action["steering"]
        out["act_accel"][i] = v.action["acceleration"]
        out["lane"][i] = v.lane_index[2]
        out["target_lane"][i] = getattr(v, "target_lane_index", v.lane_index)[2]
        out["speed_index"][i] = getattr(v, "speed_index", -1)
        out["crashed"][i] = v.crashed
        out["check_collisions"][i] = v.check_collisions
        out["controlled"][i] = v in env.controlled_vehicles
    return out


def discrete(**kw) -> dict:
    return dict({"type": "DiscreteAction"}, **kw)


NARROW = {"steering_range": [-0.05, 0.05]}
DENSE = {"vehicles_count": 30, "vehicles_density": 2.0, "lanes_count": 3, "ego_spacing": 1.0, "duration": 20}

SCENARIOS = [
    # the headline shape: highway-fast-v0, 50 vehicles, 4 lanes; a narrow steering range so that episodes last
    dict(name="direct_fast", cls=HighwayEnvFast, config={"vehicles_count": 50, "lanes_count": 4, "action": discrete(**NARROW)},
         seeds=[0, 1, 2, 3], steps=12, action_seed=201, frames_for=2),
    # highway-v0: 15 Hz, full pairwise collisions
    dict(name="direct_v0", cls=HighwayEnv, config={"vehicles_count": 30, "action": discrete(steering_range=[-0.1, 0.1])},
         seeds=[4, 5], steps=6, action_seed=202, frames_for=1),
    # 5 x 5 actions, a non-default (asymmetric) acceleration range
    dict(name="direct_k5", cls=HighwayEnvFast,
         config={"vehicles_count": 20, "action": discrete(actions_per_axis=5, acceleration_range=[-3.0, 2.0], **NARROW)},
         seeds=[6, 7, 8], steps=10, action_seed=203, frames_for=1),
    # constant full throttle: MAX_SPEED is passed, the clip sticks, the ego runs into its leader (the crashed branch of clip_actions)
    dict(name="direct_throttle", cls=HighwayEnvFast, config={"vehicles_count": 20, "action": discrete()},
         seeds=[0, 1, 2, 3], steps=8, constant=7, frames_for=2),
    # constant full brake at 15 Hz: through speed 0, reversing off the road start, down to MIN_SPEED and the clip there
    dict(name="direct_brake", cls=HighwayEnv, config={"vehicles_count": 20, "lanes_count": 3, "duration": 40, "action": discrete()},
         seeds=[0, 1, 2, 3], steps=20, constant=1, frames_for=1),
    # steering held to the right until the ego is off the road
    dict(name="direct_offroad", cls=HighwayEnvFast,
         config={"vehicles_count": 15, "lanes_count": 3, "action": discrete(steering_range=[-0.1, 0.1])},
         seeds=[10, 11, 12], steps=8, constant=5, frames_for=1),
    dict(name="direct_offroad_terminal", cls=HighwayEnvFast,
         config={"vehicles_count": 15, "lanes_count": 3, "offroad_terminal": True, "normalize_reward": False,
                 "action": discrete(steering_range=[-0.1, 0.1])},
         seeds=[10, 11, 12], steps=8, constant=3, frames_for=0),
    # one axis only: the other control is the integer 0
    dict(name="direct_longi_only", cls=HighwayEnvFast,
         config={"vehicles_count": 20, "action": discrete(lateral=False, actions_per_axis=4)},
         seeds=[13, 14, 15], steps=10, action_seed=204, frames_for=1),
    dict(name="direct_lat_only", cls=HighwayEnvFast,
         config={"vehicles_count": 20, "lanes_count": 4, "action": discrete(longitudinal=False, **NARROW)},
         seeds=[16, 17, 18], steps=10, action_seed=205, frames_for=1),
    # two agents
    dict(name="direct_ma2", cls=HighwayEnvFast,
         config={"vehicles_count": 30, "lanes_count": 3, "controlled_vehicles": 2,
                 "observation": {"type": "MultiAgentObservation", "observation_config": {"type": "Kinematics"}},
                 "action": {"type": "MultiAgentAction", "action_config": discrete(**NARROW)}},
         seeds=[19, 20], steps=10, action_seed=206, frames_for=1),
    # N = 101: two wavefronts per environment on the workgroup kernel
    dict(name="direct_n100", cls=HighwayEnv, config={"vehicles_count": 100, "action": discrete(**NARROW)},
         seeds=[21, 22], steps=3, action_seed=207, frames_for=1),
    # many first crashes, compared in full (tests/test_collision_steps.py's method): dense traffic, the default +-pi/4 steering
    dict(name="direct_crash_many", cls=HighwayEnvFast, config=dict(DENSE, action=discrete(steering_range=[-0.2, 0.2])),
         seeds=list(range(400, 424)), steps=10, action_seed=208, frames_for=0),
    # the ego leaves a lane within a policy step while a vehicle behind it is on its way INTO that lane: with the ego counted as
    # a rival of the abort rule (behavior.py:229-244) that lane change is given up.  Seeds and action sequences found by a search
    # over 400 seeds with the emulation of the kernels, intact against such a build (tests/test_control_mutations.py).
    dict(name="direct_rival", cls=HighwayEnvFast,
         config={"vehicles_count": 30, "vehicles_density": 2.0, "lanes_count": 4, "ego_spacing": 1.0, "duration": 20,
                 "action": discrete(steering_range=[-0.1, 0.1])},
         seeds=[1241, 1273], steps=8, actions=[[7, 5], [1, 4], [4, 0], [0, 6], [7, 6], [0, 8], [7, 3], [2, 3]], frames_for=0),
]


def action_config(sc: dict) -> dict:
    act = sc["config"]["action"]
    return act["action_config"] if act["type"] == "MultiAgentAction" else act


def num_ids(sc: dict) -> int:
    act = action_config(sc)
    size = int(act.get("longitudinal", True)) + int(act.get("lateral", True))
    return int(act.get("actions_per_axis", 3)) ** size


def run(sc: dict, only_envs=None) -> dict:
    """`only_envs`: simulate only these env indices (the actions are drawn for all of them either way)."""
    ref_stub.restore_class_defaults()
    seeds, steps = sc["seeds"], sc["steps"]
    A = int(sc["config"].get("controlled_vehicles", 1))
    if "actions" in sc:  # [steps][E], single agent
        actions = np.asarray(sc["actions"], np.int32).reshape(steps, len(seeds), A)
    elif "constant" in sc:
        actions = np.full((steps, len(seeds), A), sc["constant"], np.int32)
    else:
        actions = np.random.default_rng(sc["action_seed"]).integers(0, num_ids(sc), size=(steps, len(seeds), A)).astype(np.int32)
    out = {"seeds": np.asarray(seeds, np.int64), "actions": actions}
    recs = []
    for e, seed in enumerate(seeds):
        if only_envs is not None and e not in only_envs:
            continue
        env = sc["cls"](dict(sc["config"]))
        obs0, _ = env.reset(seed=int(seed))
        rec = {"obs0": np.stack(obs0) if A > 1 else obs0[None], "init": dump_state(env), "obs": [], "reward": [], "terminated": [],
               "truncated": [], "step_state": [], "frames": []}
        if e < sc["frames_for"]:
            orig = env.road.step

            def step_and_dump(dt, _orig=orig, _env=env, _rec=rec):
                _orig(dt)
                _rec["frames"].append(dump_state(_env))

            env.road.step = step_and_dump
        for t in range(steps):
            a = tuple(int(v) for v in actions[t, e]) if A > 1 else int(actions[t, e, 0])
            o, r, te, tr, info = env.step(a)
            rec["obs"].append(np.stack(o) if A > 1 else o[None])
            rec["reward"].append(r)
            rec["terminated"].append(te)
            rec["truncated"].append(tr)
            rec["step_state"].append(dump_state(env))
        rec["T"] = int(env.config["simulation_frequency"] // env.config["policy_frequency"])
        rec["cfg"] = dict(env.config)
        recs.append(rec)
    # the table DiscreteAction.act builds (action.py:190-194) and what get_action maps it to, from the last environment's action type
    at = env.action_type
    at = at.agents_action_types[0] if A > 1 else at
    cont = super(type(at), at).space()
    axes = np.linspace(cont.low, cont.high, at.actions_per_axis).T
    all_actions = list(itertools.product(*axes))
    out["all_actions"] = np.asarray(all_actions)
    assert out["all_actions"].dtype == np.float32, out["all_actions"].dtype
    mapped = [at.get_action(np.asarray(a)) for a in all_actions]
    out["axis_accel"] = np.asarray([float(m["acceleration"]) for m in mapped], np.float64)   # per action id
    out["axis_steer"] = np.asarray([float(m["steering"]) for m in mapped], np.float64)
    cfg = recs[0]["cfg"]
    out["meta"] = np.asarray([len(recs), len(recs[0]["init"]["x"]), recs[0]["T"], steps, sc["frames_for"]], np.int64)
    for k in ("lanes_count", "vehicles_count", "simulation_frequency", "policy_frequency", "normalize_reward", "offroad_terminal"):
        out["cfg_" + k] = np.int64(cfg[k])
    for k in ("duration", "ego_spacing", "vehicles_density", "collision_reward", "right_lane_reward", "high_speed_reward"):
        out["cfg_" + k] = np.float64(cfg[k])
    out["cfg_reward_speed_range"] = np.asarray(cfg["reward_speed_range"], np.float64)
    out["cfg_fast"] = np.int64(sc["cls"] is HighwayEnvFast)
    out["cfg_controlled_vehicles"] = np.int64(A)
    out["cfg_observation_json"] = np.asarray(json.dumps(cfg["observation"]))
    out["cfg_action_json"] = np.asarray(json.dumps(cfg["action"]))
    out["obs0"] = np.stack([r["obs0"] for r in recs])                                   # [E, A, V, F]
    out["obs"] = np.stack([np.stack(r["obs"]) for r in recs], axis=1)                   # [steps, E, A, V, F]
    out["reward"] = np.asarray([r["reward"] for r in recs], np.float64).T               # [steps, E]
    out["terminated"] = np.asarray([r["terminated"] for r in recs], np.int8).T
    out["truncated"] = np.asarray([r["truncated"] for r in recs], np.int8).T
    for k in F64_FIELDS + I8_FIELDS:
        out["init_" + k] = np.stack([r["init"][k] for r in recs])
        out["step_" + k] = np.stack([np.stack([s[k] for s in r["step_state"]]) for r in recs], axis=1)
        if sc["frames_for"]:
            out["frame_" + k] = np.stack([np.stack([s[k] for s in r["frames"]]) for r in recs[:sc["frames_for"]]], axis=1)
    return out


def digest(data) -> str:
    """sha256 over the arrays of a fixture (names, dtypes, shapes and raw bytes in name order): independent of the zip container."""
    h = hashlib.sha256()
    for k in sorted(data.files if hasattr(data, "files") else data):
        a = np.asarray(data[k])
        h.update(k.encode())
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main() -> None:
    only = set(sys.argv[1:])
    mpath = os.path.join(HERE, "MANIFEST.json")
    manifest = json.load(open(mpath)) if os.path.exists(mpath) else {}
    for sc in SCENARIOS:
        if only and sc["name"] not in only:
            continue
        data = run(sc)
        path = os.path.join(HERE, sc["name"] + ".npz")
        np.savez_compressed(path, **data)
        with np.load(path) as z:
            manifest[sc["name"]] = digest(z)
        ego = data["step_speed"][:, :, 0]
        print(f"{sc['name']}: E,N,T,steps,frames_for={data['meta'].tolist()} terminated={int(data['terminated'].any(0).sum())} "
              f"ego speed {ego.min():.3f}..{ego.max():.3f} -> {os.path.getsize(path) / 1024:.0f} KiB")
    with open(mpath, "w") as fh:
        json.dump(dict(sorted(manifest.items())), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
