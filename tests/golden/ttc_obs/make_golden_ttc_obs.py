#!/usr/bin/env python3
"""Generate the TimeToCollision observation fixtures in this directory from the UNMODIFIED reference.

TEST INFRASTRUCTURE.  Needs the reference package (``HWY_REFERENCE_ROOT``), imported through ``oracle/ref_stub.py`` like the
other generators:

    python tests/golden/ttc_obs/make_golden_ttc_obs.py [fixture ...]

Each fixture records a ``HighwayEnv`` / ``HighwayEnvFast`` run configured with ``{"type": "TimeToCollision", "horizon": h}`` (two
agents: wrapped in ``MultiAgentObservation``): the state at reset and after every step (tests/golden/control/make_golden_control.py's
record of a vehicle), what ``env.reset()`` / ``env.step()`` returned as the observation -- ``observe()`` of every controlled vehicle,
``obs0`` float32 [E, A, 3, 3, T] and ``obs`` [steps, E, A, 3, 3, T] -- and the reference's ``compute_ttc_grid`` of the same states
(``grid0`` / ``grid``), which the knife-edge check below restates.  Actions are drawn at random, or scripted per environment
(``script``: repeated LANE_LEFT / LANE_RIGHT / FASTER / SLOWER drive the ego to the edges of the road and of the speed ladder; the
generator asserts that it got there).

No fixture holds a knife edge: for every candidate (other vehicle, ego speed, collision point) with q = ttc / tq < T + 1 the
generator asserts |q - rint(q)| >= 1e-9 (tests/ttc_util.py: restate_grid, through make_golden_ttc.py's assert_no_knife_edge).  The
digests of the arrays go to ``MANIFEST.json`` here.
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
sys.path.insert(0, os.path.join(GOLDEN, "ttc"))

import make_golden_control as mgc  # noqa: E402  (installs the reference stub, gymnasium's array Box, imports the reference)
import make_golden_ttc as mgt  # noqa: E402  (config_record, behavior_of, assert_no_knife_edge)
from oracle import ref_stub  # noqa: E402

from highway_env.envs.common.finite_mdp import compute_ttc_grid  # noqa: E402
from highway_env.envs.highway_env import HighwayEnv, HighwayEnvFast  # noqa: E402

LEFT, IDLE, RIGHT, FASTER, SLOWER = range(5)


def ttc(horizon: float = 10.0) -> dict:
    return {"observation": {"type": "TimeToCollision", "horizon": horizon}}


def speeds(values) -> dict:
    return {"action": {"type": "DiscreteMetaAction", "target_speeds": [float(v) for v in values]}}


MA = {"observation": {"type": "MultiAgentObservation", "observation_config": {"type": "TimeToCollision", "horizon": 10.0}},
      "action": {"type": "MultiAgentAction", "action_config": {"type": "DiscreteMetaAction"}}}
DENSE = {"vehicles_count": 30, "vehicles_density": 2.0, "lanes_count": 3, "ego_spacing": 1.0, "duration": 20}

SCENARIOS = [
    # highway-fast-v0 as it comes: 3 lanes, 3 speeds, T = 10
    dict(name="ttcobs_fast", cls=HighwayEnvFast, config=dict(ttc()), seeds=[0, 1, 2], steps=5, action_seed=501),
    # one lane: both side lanes are padding
    dict(name="ttcobs_lanes1", cls=HighwayEnvFast, config=dict(ttc(), lanes_count=1, vehicles_count=10), seeds=[4, 6], steps=4, action_seed=502),
    # two lanes: one side lane is always padding
    dict(name="ttcobs_lanes2", cls=HighwayEnvFast, config=dict(ttc(), lanes_count=2, vehicles_count=14), seeds=[6, 7], steps=5, action_seed=503),
    # sixteen lanes: every bit of the packed lane index, most vehicles outside the window
    dict(name="ttcobs_lanes16", cls=HighwayEnvFast, config=dict(ttc(), lanes_count=16, vehicles_count=60), seeds=[8, 9], steps=3, action_seed=504),
    # 2 target speeds (every window holds a repeated row) and 8
    dict(name="ttcobs_speeds2", cls=HighwayEnvFast, config=dict(ttc(), **speeds([18, 28])), seeds=[10, 11], steps=5, action_seed=505),
    dict(name="ttcobs_speeds8", cls=HighwayEnvFast, config=dict(ttc(), lanes_count=4, **speeds(range(12, 34, 3))), seeds=[12, 13], steps=5,
         action_seed=506),
    # T = 1 (horizon 1 s at 1 Hz), T = 50 (policy_frequency 5) and T = 64 (horizon 64 s at 1 Hz)
    dict(name="ttcobs_horizon1", cls=HighwayEnvFast, config=dict(ttc(1.0)), seeds=[14, 15], steps=3, action_seed=507, horizon=1.0),
    dict(name="ttcobs_pf5", cls=HighwayEnv, config=dict(ttc(), policy_frequency=5, vehicles_count=30), seeds=[16, 17], steps=4, action_seed=508),
    dict(name="ttcobs_t64", cls=HighwayEnvFast, config=dict(ttc(64.0), vehicles_count=30, lanes_count=4), seeds=[18, 19], steps=3, action_seed=509,
         horizon=64.0),
    # two agents: each one's window, the other agent as an obstacle
    dict(name="ttcobs_ma2", cls=HighwayEnvFast,
         config=dict(MA, vehicles_count=12, lanes_count=3, controlled_vehicles=2, ego_spacing=1.0, vehicles_density=2.0),
         seeds=[22, 23, 25], steps=5, action_seed=510),
    # the ego driven to both edges of the road (environment 0 and 2: left; 1 and 3: right) ...
    dict(name="ttcobs_edges", cls=HighwayEnvFast, config=dict(ttc(), vehicles_count=12), seeds=[26, 27, 28, 29], steps=6,
         script=[LEFT, RIGHT, LEFT, RIGHT], reach="lanes"),
    # ... and to both ends of the speed ladder (0 and 2: FASTER; 1 and 3: SLOWER), five speeds
    dict(name="ttcobs_ladder", cls=HighwayEnvFast, config=dict(ttc(), vehicles_count=12, **speeds([15, 19, 23, 27, 31])), seeds=[30, 31, 32, 33],
         steps=6, script=[FASTER, SLOWER, FASTER, SLOWER], reach="speeds"),
    # crash-rich: dense traffic at 15 Hz, the observer crashed and slowing down
    dict(name="ttcobs_crash", cls=HighwayEnv, config=dict(ttc(), **DENSE), seeds=[503, 510, 512, 515], steps=6, action_seed=513, reach="crash"),
    # N = 1: no other vehicle
    dict(name="ttcobs_alone", cls=HighwayEnvFast, config=dict(ttc(), vehicles_count=0), seeds=[34, 35], steps=3, action_seed=514),
]
NAMES = [sc["name"] for sc in SCENARIOS]


def observed(obs, A: int) -> np.ndarray:
    """What reset() / step() returned -> float32 [A, 3, 3, T]."""
    out = np.stack([np.asarray(o) for o in obs]) if A > 1 else np.asarray(obs)[None]
    assert out.dtype == np.float32 and out.shape[:3] == (A, 3, 3), (out.dtype, out.shape)
    return out


def run(sc: dict) -> dict:
    ref_stub.restore_class_defaults()
    seeds, steps = list(sc["seeds"]), sc["steps"]
    horizon = float(sc.get("horizon", mgt.HORIZON))
    A = int(sc["config"].get("controlled_vehicles", 1))
    if "script" in sc:
        actions = np.broadcast_to(np.asarray(sc["script"], np.int32)[None, :, None], (steps, len(seeds), A)).copy()
    else:
        actions = np.random.default_rng(sc["action_seed"]).integers(0, 5, size=(steps, len(seeds), A)).astype(np.int32)
    out = {"seeds": np.asarray(seeds, np.int64), "actions": actions}
    recs = []
    for e, seed in enumerate(seeds):
        env = sc["cls"](dict(sc["config"]))
        obs, _ = env.reset(seed=int(seed))
        tq = 1 / env.config["policy_frequency"]
        grid_of = lambda: np.stack([compute_ttc_grid(env, tq, horizon, vehicle=v) for v in env.controlled_vehicles])  # noqa: E731
        rec = {"init": mgc.dump_state(env), "behavior": mgt.behavior_of(env), "obs0": observed(obs, A), "grid0": grid_of(), "obs": [], "grid": [],
               "step_state": []}
        for t in range(steps):
            obs, *_ = env.step(tuple(int(v) for v in actions[t, e]) if A > 1 else int(actions[t, e, 0]))
            rec["step_state"].append(mgc.dump_state(env))
            rec["obs"].append(observed(obs, A))
            rec["grid"].append(grid_of())
        rec["T"] = int(env.config["simulation_frequency"] // env.config["policy_frequency"])
        rec["cfg"] = dict(env.config)
        recs.append(rec)
    out["meta"] = np.asarray([len(recs), len(recs[0]["init"]["x"]), recs[0]["T"], steps, 0], np.int64)
    mgt.config_record(out, recs[0]["cfg"], sc["cls"], A, horizon)
    out["init_behavior"] = np.stack([r["behavior"] for r in recs])
    for k in ("obs", "grid"):
        out[k + "0"] = np.stack([r[k + "0"] for r in recs])                                  # [E, A, ...]
        out[k] = np.stack([np.stack(r[k]) for r in recs], axis=1)                            # [steps, E, A, ...]
    for k in mgc.F64_FIELDS + mgc.I8_FIELDS:
        out["init_" + k] = np.stack([r["init"][k] for r in recs])
        out["step_" + k] = np.stack([np.stack([s[k] for s in r["step_state"]]) for r in recs], axis=1)
    return out


def assert_reached(sc: dict, out: dict) -> None:
    """A scripted run got where its script drives it; a crash run crashes."""
    reach = sc.get("reach")
    ego = np.flatnonzero(out["init_controlled"][0])[0]
    if reach == "lanes":
        lanes = out["step_lane"][:, :, ego]
        assert lanes.min() == 0 and lanes.max() == int(out["cfg_lanes_count"]) - 1, lanes
    elif reach == "speeds":
        idx, top = out["step_speed_index"][:, :, ego], len(json.loads(str(out["cfg_action_json"]))["target_speeds"]) - 1
        assert idx.min() == 0 and idx.max() == top, idx
    elif reach == "crash":
        assert out["step_crashed"][:, :, ego].any(), "no observer crashed"


def main() -> None:
    only = set(sys.argv[1:])
    mpath = os.path.join(HERE, "MANIFEST.json")
    manifest = json.load(open(mpath)) if os.path.exists(mpath) else {}
    for sc in SCENARIOS:
        name = sc["name"]
        if only and name not in only:
            continue
        data = run(sc)
        assert_reached(sc, data)
        # (the restatement needs an engine config: the Kinematics observation stands in for the type the engine rejects)
        check = dict(data)
        check["cfg_observation_json"] = np.asarray(json.dumps(mgt.MA["observation"] if "controlled_vehicles" in sc["config"] else {"type": "Kinematics"}))
        closest = mgt.assert_no_knife_edge(check, name)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **data)
        with np.load(path) as z:
            manifest[name] = mgc.digest(z)
        print(f"{name}: E,N,T,steps={data['meta'][:4].tolist()} obs {data['obs0'].shape[1:]} marked cells {(data['obs'] > 0).mean():.3f} "
              f"closest candidate to a boundary {closest:.3g} -> {os.path.getsize(path) / 1024:.0f} KiB")
    with open(mpath, "w") as fh:
        json.dump(dict(sorted(manifest.items())), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
