#!/usr/bin/env python3
"""Generate the continuous-control (``ContinuousAction``) fixtures in this directory from the UNMODIFIED reference.

TEST INFRASTRUCTURE.  Needs the reference package (``HWY_REFERENCE_ROOT``), imported through ``oracle/ref_stub.py`` like the
other generators:

    python tests/golden/continuous/make_golden_continuous.py [fixture ...]

Each fixture records a ``HighwayEnv`` / ``HighwayEnvFast`` run whose ``config["action"]`` is a ``ContinuousAction`` (or a
``MultiAgentAction`` over one), driven with float32 actions: the record of tests/golden/control/make_golden_control.py (whose
``dump_state`` this generator uses: the state, and every vehicle's stored action AFTER ``clip_actions`` wrote into it, after every
frame of the first ``frames_for`` environments and after every step), with
  ``actions``        float32 [steps, E, A, size]  what ``env.step`` was given (``Box(-1, 1, (size,), float32)``'s dtype; random ones
                                                  are drawn from [-1.3, 1.3], so that ``np.clip`` works)
  ``mapped_accel``   float64 [steps, E, A]        ``float()`` of what the reference's own ``get_action`` returned for them: the pair
  ``mapped_steer``   float64 [steps, E, A]        ``Vehicle.act`` stored BEFORE ``clip_actions`` rewrote it on the first frame
The digests of the arrays go to ``MANIFEST.json`` here.  For every fixture the generator prints the counts the tests lean on:
environments that terminate, (step, environment, agent) entries whose stored action ``clip_actions`` rewrote within the step
(the others are compared bit for bit with the engine's stored controls) and the range of the ego's speed.
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

from oracle import ref_stub  # noqa: E402
from highway_env.envs.highway_env import HighwayEnv, HighwayEnvFast  # noqa: E402

dump_state, digest, F64_FIELDS, I8_FIELDS = control.dump_state, control.digest, control.F64_FIELDS, control.I8_FIELDS


def continuous(**kw) -> dict:
    return dict({"type": "ContinuousAction"}, **kw)


NARROW = {"steering_range": [-0.05, 0.05]}
DENSE = {"vehicles_count": 30, "vehicles_density": 2.0, "lanes_count": 3, "ego_spacing": 1.0, "duration": 20}

SCENARIOS = [
    # the headline shape: highway-fast-v0, 50 vehicles, 4 lanes; a narrow steering range so that episodes last
    dict(name="cont_fast", cls=HighwayEnvFast, config={"vehicles_count": 50, "lanes_count": 4, "action": continuous(**NARROW)},
         seeds=[0, 1, 2, 3], steps=12, action_seed=301, frames_for=2),
    # highway-v0: 15 Hz, full pairwise collisions
    dict(name="cont_v0", cls=HighwayEnv, config={"vehicles_count": 30, "action": continuous(steering_range=[-0.1, 0.1])},
         seeds=[4, 5], steps=6, action_seed=302, frames_for=1),
    # asymmetric ranges whose ends are not float32 numbers: the rounding of (y1 - y0) and of y0 shows
    dict(name="cont_asym", cls=HighwayEnvFast,
         config={"vehicles_count": 20, "action": continuous(acceleration_range=[-3.3, 2.1], steering_range=[-0.3, 0.1])},
         seeds=[6, 7, 8], steps=10, action_seed=303, frames_for=1),
    # one axis only: the other control is the integer 0, the action has one component
    dict(name="cont_longi_only", cls=HighwayEnvFast, config={"vehicles_count": 20, "action": continuous(lateral=False)},
         seeds=[13, 14, 15], steps=10, action_seed=304, frames_for=1),
    dict(name="cont_lat_only", cls=HighwayEnvFast,
         config={"vehicles_count": 20, "lanes_count": 4, "action": continuous(longitudinal=False, **NARROW)},
         seeds=[16, 17, 18], steps=10, action_seed=305, frames_for=1),
    # two agents
    dict(name="cont_ma2", cls=HighwayEnvFast,
         config={"vehicles_count": 30, "lanes_count": 3, "controlled_vehicles": 2,
                 "observation": {"type": "MultiAgentObservation", "observation_config": {"type": "Kinematics"}},
                 "action": {"type": "MultiAgentAction", "action_config": continuous(**NARROW)}},
         seeds=[19, 20], steps=10, action_seed=306, frames_for=1),
    # N = 101: two wavefronts per environment on the workgroup kernel
    dict(name="cont_n100", cls=HighwayEnv, config={"vehicles_count": 100, "action": continuous(**NARROW)},
         seeds=[21, 22], steps=3, action_seed=307, frames_for=1),
    # constant full throttle (beyond the clip), straight: MAX_SPEED is passed, clip_actions rewrites the stored acceleration and it
    # sticks, the ego runs into its leader (the crashed branch of clip_actions)
    dict(name="cont_throttle", cls=HighwayEnvFast, config={"vehicles_count": 20, "action": continuous()},
         seeds=[0, 1, 2, 3], steps=8, constant=[1.25, 0.0], frames_for=2),
    # many first crashes, compared in full: dense traffic, a wide steering range
    dict(name="cont_dense", cls=HighwayEnvFast, config=dict(DENSE, action=continuous(steering_range=[-0.2, 0.2])),
         seeds=list(range(400, 424)), steps=10, action_seed=308, frames_for=0),
]


def action_config(sc: dict) -> dict:
    act = sc["config"]["action"]
    return act["action_config"] if act["type"] == "MultiAgentAction" else act


def action_size(sc: dict) -> int:
    act = action_config(sc)
    return int(act.get("longitudinal", True)) + int(act.get("lateral", True))


def run(sc: dict, only_envs=None) -> dict:
    """`only_envs`: simulate only these env indices (the actions are drawn for all of them either way)."""
    ref_stub.restore_class_defaults()
    seeds, steps = sc["seeds"], sc["steps"]
    A, size = int(sc["config"].get("controlled_vehicles", 1)), action_size(sc)
    if "constant" in sc:
        actions = np.broadcast_to(np.asarray(sc["constant"], np.float32)[:size], (steps, len(seeds), A, size)).copy()
    else:
        actions = np.random.default_rng(sc["action_seed"]).uniform(-1.3, 1.3, size=(steps, len(seeds), A, size)).astype(np.float32)
    out = {"seeds": np.asarray(seeds, np.int64), "actions": actions}
    recs = []
    for e, seed in enumerate(seeds):
        if only_envs is not None and e not in only_envs:
            continue
        env = sc["cls"](dict(sc["config"]))
        obs0, _ = env.reset(seed=int(seed))
        rec = {"obs0": np.stack(obs0) if A > 1 else obs0[None], "init": dump_state(env), "obs": [], "reward": [], "terminated": [],
               "truncated": [], "step_state": [], "frames": [], "mapped": []}
        if e < sc["frames_for"]:
            orig = env.road.step

            def step_and_dump(dt, _orig=orig, _env=env, _rec=rec):
                _orig(dt)
                _rec["frames"].append(dump_state(_env))

            env.road.step = step_and_dump
        types = env.action_type.agents_action_types if A > 1 else [env.action_type]
        for t in range(steps):
            a = tuple(actions[t, e, k].copy() for k in range(A)) if A > 1 else actions[t, e, 0].copy()
            mapped = [at.get_action(actions[t, e, k].copy()) for k, at in enumerate(types)]  # (pure: speed_range is None)
            rec["mapped"].append([[float(m["acceleration"]), float(m["steering"])] for m in mapped])
            o, r, te, tr, info = env.step(a)
            rec["obs"].append(np.stack(o) if A > 1 else o[None])
            rec["reward"].append(r)
            rec["terminated"].append(te)
            rec["truncated"].append(tr)
            rec["step_state"].append(dump_state(env))
        rec["T"] = int(env.config["simulation_frequency"] // env.config["policy_frequency"])
        rec["cfg"] = dict(env.config)
        recs.append(rec)
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
    mapped = np.asarray([r["mapped"] for r in recs], np.float64).transpose(1, 0, 2, 3)  # [steps, E, A, 2]
    out["mapped_accel"], out["mapped_steer"] = np.ascontiguousarray(mapped[..., 0]), np.ascontiguousarray(mapped[..., 1])
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


def rewritten(data) -> np.ndarray:
    """bool [steps, E, A]: ``clip_actions`` rewrote the agent's stored action within the step (the stored pair after the step is not
    the pair ``get_action`` mapped the action to)."""
    agents = np.flatnonzero(np.asarray(data["init_controlled"])[0])
    return (np.asarray(data["step_act_accel"])[:, :, agents] != data["mapped_accel"]) | (
        np.asarray(data["step_act_steering"])[:, :, agents] != data["mapped_steer"])


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
        ego = data["step_speed"][:, :, np.flatnonzero(data["init_controlled"][0])]
        rw = rewritten(data)
        print(f"{sc['name']}: E,N,T,steps,frames_for={data['meta'].tolist()} terminated={int(data['terminated'].any(0).sum())} "
              f"rewritten by clip_actions={int(rw.sum())}/{rw.size} ego speed {ego.min():.3f}..{ego.max():.3f} "
              f"-> {os.path.getsize(path) / 1024:.0f} KiB")
    with open(mpath, "w") as fh:
        json.dump(dict(sorted(manifest.items())), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
