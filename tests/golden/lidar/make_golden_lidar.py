#!/usr/bin/env python3
"""Generate the ``LidarObservation`` fixtures in this directory from the UNMODIFIED reference.

TEST INFRASTRUCTURE.  Needs the reference package (``HWY_REFERENCE_ROOT``), imported through ``oracle/ref_stub.py`` like the
other generators:

    python tests/golden/lidar/make_golden_lidar.py [fixture ...]

Each fixture records a ``HighwayEnv`` / ``HighwayEnvFast`` run whose ``config["observation"]`` is a ``LidarObservation`` (alone or
under ``MultiAgentObservation``): the initial state and the state after every step (tests/golden/control/make_golden_control.py's
record of a vehicle, which covers MDPVehicle, plain Vehicle and IDM / Linear traffic), the reference's lidar observation at reset
(``obs0`` [E, A, cells, 2]) and after every step (``obs`` [steps, E, A, cells, 2]), reward / terminated / truncated, and for
LinearVehicle traffic the parameters ``randomize_behavior`` drew (``init_behavior`` [E, N, 5]).

``lidar_crafted`` is not a run: every environment is a hand-placed road (CRAFTED below), written onto the vehicles of a reference
environment, and ``obs0`` is the reference's ``observe()`` of it -- ``steps`` is 0.  README.md says what each road is for.
The digests of the arrays go to ``MANIFEST.json`` here.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(GOLDEN, "control"))

import make_golden_control as mgc  # noqa: E402  (installs the reference stub, gymnasium's array Box, imports the reference)
from oracle import ref_stub  # noqa: E402

from highway_env.envs.highway_env import HighwayEnv, HighwayEnvFast  # noqa: E402
from highway_env.vehicle.behavior import LinearVehicle  # noqa: E402

LINEAR = "highway_env.vehicle.behavior.LinearVehicle"


def lidar(**kw) -> dict:
    return dict({"type": "LidarObservation"}, **kw)


SCENARIOS = [
    # the headline shape: highway-fast-v0, 50 vehicles, 4 lanes, 16 cells
    dict(name="lidar_fast", cls=HighwayEnvFast, config={"vehicles_count": 50, "lanes_count": 4, "observation": lidar(cells=16)},
         seeds=[0, 1, 2, 3], steps=12, action_seed=301),
    # highway-v0: 15 Hz, every vehicle checks collisions
    dict(name="lidar_v0", cls=HighwayEnv, config={"vehicles_count": 30, "observation": lidar()}, seeds=[4, 5, 6], steps=8,
         action_seed=302),
    # 64 cells (every lane of the wavefront holds a cell), raw distances, a short range: most traffic is beyond it
    dict(name="lidar_cells64_raw", cls=HighwayEnvFast,
         config={"vehicles_count": 40, "lanes_count": 4, "observation": lidar(cells=64, maximum_range=35, normalize=False)},
         seeds=[7, 8, 9], steps=10, action_seed=303),
    # two agents observing each other (the second ego is spawned behind the first one's share of the traffic: within range)
    dict(name="lidar_ma2", cls=HighwayEnvFast,
         config={"vehicles_count": 12, "lanes_count": 3, "controlled_vehicles": 2, "ego_spacing": 1.0, "vehicles_density": 2.0,
                 "observation": {"type": "MultiAgentObservation", "observation_config": lidar(cells=24, maximum_range=120)},
                 "action": {"type": "MultiAgentAction", "action_config": {"type": "DiscreteMetaAction"}}},
         seeds=[10, 11, 12], steps=10, action_seed=304),
    # N = 101: two passes of 64 obstacles
    dict(name="lidar_n100", cls=HighwayEnv, config={"vehicles_count": 100, "observation": lidar(cells=32, maximum_range=120)},
         seeds=[13, 14], steps=3, action_seed=305),
    # LinearVehicle traffic
    dict(name="lidar_linear", cls=HighwayEnvFast,
         config={"vehicles_count": 40, "lanes_count": 4, "other_vehicles_type": LINEAR, "observation": lidar(cells=20)},
         seeds=[15, 16, 17], steps=10, action_seed=306),
    # DiscreteAction ego: steering held until the heading is far from 0
    dict(name="lidar_direct", cls=HighwayEnvFast,
         config={"vehicles_count": 30, "lanes_count": 4, "observation": lidar(cells=16),
                 "action": {"type": "DiscreteAction", "steering_range": [-0.15, 0.15]}},
         seeds=[18, 19, 20], steps=8, actions=[[5, 3, 8]] * 3 + [[3, 5, 6]] * 3 + [[4, 4, 4]] * 2),
    # dense traffic at 15 Hz with full pairwise collisions: overlapping rectangles, negative centre distances
    dict(name="lidar_crash", cls=HighwayEnv,
         config={"vehicles_count": 30, "vehicles_density": 2.0, "lanes_count": 3, "ego_spacing": 1.0, "duration": 20,
                 "observation": lidar(cells=16, maximum_range=40)},
         seeds=list(range(500, 512)), steps=6, action_seed=308),
]

# ---- lidar_crafted: hand-placed roads --------------------------------------------------------------------------------------------
# cells 16 (cell k looks along k * 22.5 degrees, cell 0 spans +-11.25 degrees), maximum_range 60, raw values.  Slot 0 is the
# observer at (100, 4), heading 0, 25 m/s; each obstacle is (x, y, heading, speed); the slots a road does not use stand far away.
OBSERVER = (100.0, 4.0, 0.0, 25.0)
CRAFTED = [
    # 0  exact tie, same rectangle twice with different speeds: the LATER obstacle's velocity survives in every cell
    [(120.0, 4.0, 0.0, 20.0), (120.0, 4.0, 0.0, 30.0)],
    # 1  exact tie of the centre candidates of two mirrored obstacles in cell 0 (equal centre distances)
    [(130.0, 4.25, 0.0, 21.0), (130.0, 3.75, 0.0, 28.0)],
    # 2  30 m and 30 m + 1e-9 ahead, the nearer one first: the second is above the stored float32 and loses
    [(130.0, 4.0, 0.0, 20.0), (130.0 + 1e-9, 4.0, 0.0, 30.0)],
    # 3  ... the farther one first: stored as float32(29.000000001) = 29, which the nearer one ties with `<=`
    [(130.0 + 1e-9, 4.0, 0.0, 30.0), (130.0, 4.0, 0.0, 20.0)],
    # 4  the same rectangle at 30 m + 1e-9 twice: the second lies above the ROUNDED stored value and loses (an f64 fold takes it)
    [(130.0 + 1e-9, 4.0, 0.0, 30.0), (130.0 + 1e-9, 4.0, 0.0, 20.0)],
    # 5  centre 60.5 m ahead (beyond range), rear corners at 58 m: skipped entirely
    [(160.5, 4.0, 0.0, 22.0)],
    # 6  ... and 59.9 m: traced
    [(159.9, 4.0, 0.0, 22.0)],
    # 7  straight behind, heading exactly 0: the corners straddle +-pi
    [(80.0, 4.0, 0.0, 29.0)],
    # 8  behind and one lane to the left / right: corners on one side of +-pi
    [(75.0, 0.0, 0.0, 27.0), (85.0, 8.0, 0.0, 23.0)],
    # 9  around the boundary between cell 15 and cell 0 (-11.25 degrees): start = 15 >= end = 0; the ray of cell 0 passes it by
    [(120.0, 0.0, 0.0, 24.0)],
    # 10 level with the observer, heading exactly 0, on both sides
    [(100.0, 8.0, 0.0, 26.0), (100.0, 0.0, 0.0, 24.0)],
    # 11 ahead, behind and level at once, all headings exactly 0
    [(112.0, 4.0, 0.0, 20.0), (90.0, 4.0, 0.0, 30.0), (101.0, 8.0, 0.0, 25.0), (99.0, 0.0, 0.0, 25.0)],
    # 12 rotated rectangles
    [(110.0, 0.0, 0.7, 18.0), (95.0, 9.0, -1.2, 15.0), (104.0, 12.0, 2.9, 12.0)],
    # 13 overlapping the observer: negative centre distance
    [(100.3, 4.2, 0.05, 0.0), (103.0, 5.0, -0.3, 3.0)],
    # 14 a near obstacle that hides a far one in the same cells
    [(140.0, 4.0, 0.0, 30.0), (110.0, 4.5, 0.0, 15.0)],
    # 15 nothing in range
    [],
    # 16 close by on the right: the sector runs from cell 14 over cell 15 into cell 0, and the rays of cells 15 and 0 both hit
    [(104.0, 3.2, 0.0, 24.0)],
]
CRAFTED_SLOTS = 8


def behavior_of(env) -> np.ndarray:
    out = np.zeros((len(env.road.vehicles), 5))
    for i, v in enumerate(env.road.vehicles):
        if isinstance(v, LinearVehicle):
            out[i, :3], out[i, 3:] = v.ACCELERATION_PARAMETERS, v.STEERING_PARAMETERS
    return out


def config_record(out: dict, cfg: dict, cls, A: int) -> None:
    for k in ("lanes_count", "vehicles_count", "simulation_frequency", "policy_frequency", "normalize_reward", "offroad_terminal"):
        out["cfg_" + k] = np.int64(cfg[k])
    for k in ("duration", "ego_spacing", "vehicles_density", "collision_reward", "right_lane_reward", "high_speed_reward"):
        out["cfg_" + k] = np.float64(cfg[k])
    out["cfg_reward_speed_range"] = np.asarray(cfg["reward_speed_range"], np.float64)
    out["cfg_fast"] = np.int64(cls is HighwayEnvFast)
    out["cfg_controlled_vehicles"] = np.int64(A)
    out["cfg_other_vehicles_type"] = np.asarray(cfg["other_vehicles_type"])
    out["cfg_observation_json"] = np.asarray(json.dumps(cfg["observation"]))
    out["cfg_action_json"] = np.asarray(json.dumps(cfg["action"]))


def observation(env, A: int) -> np.ndarray:
    o = env.observation_type.observe()
    return np.stack(o) if A > 1 else np.asarray(o)[None]


def num_ids(sc: dict) -> int:
    act = sc["config"].get("action", {"type": "DiscreteMetaAction"})
    act = act.get("action_config", act)
    return mgc.num_ids(sc) if act["type"] == "DiscreteAction" else 5


def run(sc: dict, only_envs=None) -> dict:
    """`only_envs`: simulate only these env indices (the actions are drawn for all of them either way)."""
    ref_stub.restore_class_defaults()
    seeds, steps = sc["seeds"], sc["steps"]
    A = int(sc["config"].get("controlled_vehicles", 1))
    if "actions" in sc:
        actions = np.asarray(sc["actions"], np.int32).reshape(steps, len(seeds), A)
    else:
        actions = np.random.default_rng(sc["action_seed"]).integers(0, num_ids(sc), size=(steps, len(seeds), A)).astype(np.int32)
    out = {"seeds": np.asarray(seeds, np.int64), "actions": actions}
    recs = []
    for e, seed in enumerate(seeds):
        if only_envs is not None and e not in only_envs:
            continue
        env = sc["cls"](dict(sc["config"]))
        obs0, _ = env.reset(seed=int(seed))
        rec = {"obs0": np.stack(obs0) if A > 1 else obs0[None], "init": mgc.dump_state(env), "behavior": behavior_of(env), "obs": [],
               "reward": [], "terminated": [], "truncated": [], "step_state": []}
        assert rec["obs0"].dtype == np.float32
        for t in range(steps):
            a = tuple(int(v) for v in actions[t, e]) if A > 1 else int(actions[t, e, 0])
            o, r, te, tr, info = env.step(a)
            rec["obs"].append(np.stack(o) if A > 1 else o[None])
            rec["reward"].append(r)
            rec["terminated"].append(te)
            rec["truncated"].append(tr)
            rec["step_state"].append(mgc.dump_state(env))
        rec["T"] = int(env.config["simulation_frequency"] // env.config["policy_frequency"])
        rec["cfg"] = dict(env.config)
        recs.append(rec)
    out["meta"] = np.asarray([len(recs), len(recs[0]["init"]["x"]), recs[0]["T"], steps, 0], np.int64)
    config_record(out, recs[0]["cfg"], sc["cls"], A)
    out["obs0"] = np.stack([r["obs0"] for r in recs])                                   # [E, A, cells, 2]
    out["obs"] = np.stack([np.stack(r["obs"]) for r in recs], axis=1)                   # [steps, E, A, cells, 2]
    out["reward"] = np.asarray([r["reward"] for r in recs], np.float64).T               # [steps, E]
    out["terminated"] = np.asarray([r["terminated"] for r in recs], np.int8).T
    out["truncated"] = np.asarray([r["truncated"] for r in recs], np.int8).T
    out["init_behavior"] = np.stack([r["behavior"] for r in recs])
    for k in mgc.F64_FIELDS + mgc.I8_FIELDS:
        out["init_" + k] = np.stack([r["init"][k] for r in recs])
        out["step_" + k] = np.stack([np.stack([s[k] for s in r["step_state"]]) for r in recs], axis=1)
    return out


def run_crafted(only_envs=None) -> dict:
    ref_stub.restore_class_defaults()
    config = {"vehicles_count": CRAFTED_SLOTS - 1, "lanes_count": 4, "observation": lidar(cells=16, maximum_range=60, normalize=False)}
    recs = []
    for e, road in enumerate(CRAFTED):
        if only_envs is not None and e not in only_envs:
            continue
        env = HighwayEnvFast(dict(config))
        env.reset(seed=0)
        assert len(env.road.vehicles) == CRAFTED_SLOTS and env.road.vehicles[0] is env.vehicle and len(road) < CRAFTED_SLOTS
        placed = [OBSERVER] + list(road)
        placed += [(5000.0 + 100.0 * k, 0.0, 0.0, 20.0) for k in range(CRAFTED_SLOTS - len(placed))]
        for v, (x, y, h, s) in zip(env.road.vehicles, placed):
            v.position = np.array([x, y])
            v.heading, v.speed = h, s
        recs.append({"init": mgc.dump_state(env), "obs0": observation(env, 1), "cfg": dict(env.config)})
    out = {"seeds": np.zeros(len(CRAFTED), np.int64), "actions": np.zeros((0, len(CRAFTED), 1), np.int32)}
    out["meta"] = np.asarray([len(recs), CRAFTED_SLOTS, 5, 0, 0], np.int64)
    config_record(out, recs[0]["cfg"], HighwayEnvFast, 1)
    out["obs0"] = np.stack([r["obs0"] for r in recs])
    assert out["obs0"].dtype == np.float32
    for k in mgc.F64_FIELDS + mgc.I8_FIELDS:
        out["init_" + k] = np.stack([r["init"][k] for r in recs])
    return out


NAMES = [sc["name"] for sc in SCENARIOS] + ["lidar_crafted"]


def generate(name: str, only_envs=None) -> dict:
    if name == "lidar_crafted":
        return run_crafted(only_envs)
    return run(next(sc for sc in SCENARIOS if sc["name"] == name), only_envs)


def main() -> None:
    only = set(sys.argv[1:])
    mpath = os.path.join(HERE, "MANIFEST.json")
    manifest = json.load(open(mpath)) if os.path.exists(mpath) else {}
    for name in NAMES:
        if only and name not in only:
            continue
        data = generate(name)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **data)
        with np.load(path) as z:
            manifest[name] = mgc.digest(z)
        traced = (data["obs0"][..., 0] != data["obs0"][..., 0].max()).mean()
        print(f"{name}: E,N,T,steps={data['meta'][:4].tolist()} obs0 {data['obs0'].shape} traced cells at reset {traced:.2f} "
              f"terminated={int(data['terminated'].any(0).sum()) if 'terminated' in data else 0} -> {os.path.getsize(path) / 1024:.0f} KiB")
    with open(mpath, "w") as fh:
        json.dump(dict(sorted(manifest.items())), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
