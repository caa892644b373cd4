#!/usr/bin/env python3
"""Generate the LinearVehicle-family fixtures in this directory from the UNMODIFIED reference.

TEST INFRASTRUCTURE.  Needs the reference package (``HWY_REFERENCE_ROOT``), imported through ``oracle/ref_stub.py`` like the
other generators:

    python tests/golden/traffic/make_golden_traffic.py [fixture ...]

Each fixture is ``tests/golden/make_golden.py``'s record of a ``HighwayEnv`` / ``HighwayEnvFast`` run (initial state, state
after every frame for the first ``frames_for`` environments, obs / reward / terminated / truncated / info after every step) with
``config["other_vehicles_type"]`` set to a class of the LinearVehicle family, plus ``init_behavior`` [E, N, 5]: the
``ACCELERATION_PARAMETERS`` and ``STEERING_PARAMETERS`` ``randomize_behavior`` drew for every vehicle (controlled: zeros).
The digests of the arrays go to ``MANIFEST.json`` here (not ``tests/golden/MANIFEST.json``).
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
sys.path.insert(0, ROOT)
sys.path.insert(0, GOLDEN)

import make_golden as mg  # noqa: E402  (installs the reference stub and imports the reference)

LINEAR = "highway_env.vehicle.behavior.LinearVehicle"
AGGRESSIVE = "highway_env.vehicle.behavior.AggressiveVehicle"
DEFENSIVE = "highway_env.vehicle.behavior.DefensiveVehicle"
DENSE = {"vehicles_count": 30, "vehicles_density": 2.5, "lanes_count": 3, "ego_spacing": 1.0, "duration": 20}
WEAVE = [0.25, 0.05, 0.25, 0.4, 0.05]

SCENARIOS = [
    # the headline shape: highway-fast-v0, 50 vehicles, 4 lanes
    dict(name="linear_fast", cls=mg.HighwayEnvFast, config={"vehicles_count": 50, "lanes_count": 4, "other_vehicles_type": LINEAR},
         seeds=[0, 1, 2, 3], steps=12, action_seed=101, frames_for=2),
    # highway-v0: 15 Hz, full pairwise collisions
    dict(name="linear_v0", cls=mg.HighwayEnv, config={"vehicles_count": 30, "other_vehicles_type": LINEAR},
         seeds=[4, 5], steps=6, action_seed=102, frames_for=1),
    # crash-rich density, AggressiveVehicle traffic (LANE_CHANGE_MIN_ACC_GAIN = 1.0)
    dict(name="aggressive_dense", cls=mg.HighwayEnv, config=dict(DENSE, other_vehicles_type=AGGRESSIVE),
         seeds=[6, 7, 8], steps=10, action_seed=103, frames_for=2, action_p=WEAVE),
    # two controlled vehicles, DefensiveVehicle traffic
    dict(name="defensive_ma2", cls=mg.HighwayEnvFast,
         config={"vehicles_count": 30, "lanes_count": 3, "controlled_vehicles": 2, "other_vehicles_type": DEFENSIVE,
                 "observation": {"type": "MultiAgentObservation", "observation_config": {"type": "Kinematics"}},
                 "action": {"type": "MultiAgentAction", "action_config": {"type": "DiscreteMetaAction"}}},
         seeds=[9, 10], steps=10, action_seed=104, frames_for=1, multi_agent=2),
    # N = 101: two wavefronts per environment on the workgroup kernel
    dict(name="linear_n100", cls=mg.HighwayEnv, config={"vehicles_count": 100, "other_vehicles_type": LINEAR},
         seeds=[11, 12], steps=3, action_seed=105, frames_for=1),
    # many first crashes, compared in full (tests/test_collision_steps.py's method)
    dict(name="crash_many_linear", cls=mg.HighwayEnvFast, config=dict(DENSE, vehicles_density=2.0, other_vehicles_type=LINEAR),
         seeds=list(range(300, 324)), steps=10, action_seed=106, frames_for=0, action_p=WEAVE),
]


def behavior_params(sc: dict, only_envs=None) -> np.ndarray:
    """The parameters randomize_behavior drew after reset(seed) of every env: [E, N, 5], controlled vehicles zeros."""
    from highway_env.vehicle.behavior import LinearVehicle
    out = []
    for e, seed in enumerate(sc["seeds"]):
        if only_envs is not None and e not in only_envs:
            continue
        mg.ref_stub.restore_class_defaults()
        env = sc["cls"](dict(sc["config"]))
        env.reset(seed=int(seed))
        rows = []
        for v in env.road.vehicles:
            if isinstance(v, LinearVehicle):
                rows.append(np.concatenate([np.asarray(v.ACCELERATION_PARAMETERS, np.float64),
                                            np.asarray(v.STEERING_PARAMETERS, np.float64)]))
            else:
                rows.append(np.zeros(5))
        out.append(np.stack(rows))
    return np.stack(out)


def run(sc: dict, only_envs=None) -> dict:
    """`only_envs`: simulate only these env indices (the actions are drawn for all of them either way: make_golden.run_scenario)."""
    A = sc.get("multi_agent")
    if A:  # make_golden.run_scenario draws one action per env and step: a tuple of A per step here
        data = run_multi_agent(sc, A, only_envs)
    else:
        data = mg.run_scenario(sc, only_envs)
    data["init_behavior"] = behavior_params(sc, only_envs)
    data["cfg_other_vehicles_type"] = np.asarray(sc["config"]["other_vehicles_type"])
    data["cfg_controlled_vehicles"] = np.int64(A or 1)
    return data


def run_multi_agent(sc: dict, A: int, only_envs=None) -> dict:
    mg.ref_stub.restore_class_defaults()
    seeds, steps = sc["seeds"], sc["steps"]
    rng = np.random.default_rng(sc["action_seed"])
    actions = rng.integers(0, 5, size=(steps, len(seeds), A)).astype(np.int32)
    out = {"seeds": np.asarray(seeds, np.int64), "actions": actions}
    recs = []
    for e, seed in enumerate(seeds):
        if only_envs is not None and e not in only_envs:
            continue
        env = sc["cls"](dict(sc["config"]))
        obs0, _ = env.reset(seed=int(seed))
        rec = {"obs0": np.stack(obs0), "init": mg.dump_state(env), "obs": [], "reward": [], "terminated": [], "truncated": [],
               "step_state": [], "frames": []}
        if e < sc["frames_for"]:
            orig = env.road.step

            def step_and_dump(dt, _orig=orig, _env=env, _rec=rec):
                _orig(dt)
                _rec["frames"].append(mg.dump_state(_env))

            env.road.step = step_and_dump
        for t in range(steps):
            o, r, te, tr, info = env.step(tuple(int(a) for a in actions[t, e]))
            rec["obs"].append(np.stack(o))
            rec["reward"].append(r)
            rec["terminated"].append(te)
            rec["truncated"].append(tr)
            rec["step_state"].append(mg.dump_state(env))
        rec["T"] = int(env.config["simulation_frequency"] // env.config["policy_frequency"])
        rec["cfg"] = dict(env.config)
        recs.append(rec)
    cfg = recs[0]["cfg"]
    out["meta"] = np.asarray([len(recs), len(recs[0]["init"]["x"]), recs[0]["T"], steps, sc["frames_for"]], np.int64)
    for k in ("lanes_count", "vehicles_count", "simulation_frequency", "policy_frequency"):
        out["cfg_" + k] = np.int64(cfg[k])
    out["cfg_duration"] = np.float64(cfg["duration"])
    out["cfg_ego_spacing"] = np.float64(cfg["ego_spacing"])
    out["cfg_vehicles_density"] = np.float64(cfg["vehicles_density"])
    out["cfg_fast"] = np.int64(sc["cls"] is mg.HighwayEnvFast)
    out["cfg_observation_json"] = np.asarray(json.dumps(cfg["observation"]))
    out["cfg_action_json"] = np.asarray(json.dumps(cfg["action"]))
    out["obs0"] = np.stack([r["obs0"] for r in recs])
    out["obs"] = np.stack([np.stack(r["obs"]) for r in recs], axis=1)                # [steps, E, A, V, F]
    out["reward"] = np.asarray([r["reward"] for r in recs], np.float64).T
    out["terminated"] = np.asarray([r["terminated"] for r in recs], np.int8).T
    out["truncated"] = np.asarray([r["truncated"] for r in recs], np.int8).T
    for k in mg.F64_FIELDS + mg.I8_FIELDS:
        out["init_" + k] = np.stack([r["init"][k] for r in recs])
        out["step_" + k] = np.stack([np.stack([s[k] for s in r["step_state"]]) for r in recs], axis=1)
        if sc["frames_for"]:
            out["frame_" + k] = np.stack([np.stack([s[k] for s in r["frames"]]) for r in recs[:sc["frames_for"]]], axis=1)
    return out


def digest(path: str) -> str:
    """sha256 over the arrays of a fixture (names and raw bytes in name order): independent of the zip container."""
    h = hashlib.sha256()
    with np.load(path) as z:
        for k in sorted(z.files):
            a = z[k]
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
        manifest[sc["name"]] = digest(path)
        print(f"{sc['name']}: E,N,T,steps,frames_for={data['meta'].tolist()} terminated={int(data['terminated'].sum())} "
              f"-> {os.path.getsize(path) / 1024:.0f} KiB")
    with open(mpath, "w") as fh:
        json.dump(dict(sorted(manifest.items())), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
