#!/usr/bin/env python3
"""Fixtures of the float door into the planning seam, recorded from the UNMODIFIED reference: ``copy.deepcopy(env)`` followed by
``env.step`` on the copy with ``ContinuousAction`` arrays (AbstractEnv.__deepcopy__, envs/common/abstract.py:455).

TEST INFRASTRUCTURE.  Needs the reference package (``HWY_REFERENCE_ROOT``), imported through ``oracle/ref_stub.py`` like the other
generators.  The record is tests/golden/lookahead/make_golden_lookahead.py's, with float sequences:

  ``sequences``   float32 [B, K, A, size]   the candidates (drawn from [-1.3, 1.3], so that ``np.clip`` works)
  ``prev_*``, ``prev_time``, ``last_action`` float32 [E, A, size]   the state ONE step before the branch point and the action that
                                            led to it (the state an engine is loaded with to arrive at the branch point by a step
                                            of its own: a parent that terminates there then AWAITS its re-spawn)
  ``init_*``, ``branch_time``               the state at the branch point
  ``reward`` / ``terminated`` / ``truncated`` [E, B, K], ``crashed`` [E, B], ``returns`` [E, B] at ``gamma``

``until_crash`` fixtures step every environment with one constant action until the reference reports ``terminated``: the branch
point is a finished episode, and the copies go on stepping it (what stepping the reference after ``done`` gives).

    HWY_REFERENCE_ROOT=... python tests/golden/cem/make_golden_cem.py [name ...]
"""
from __future__ import annotations

import copy
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
sys.path.insert(0, os.path.join(GOLDEN, "lookahead"))

import make_golden_control as mgc  # noqa: E402  (installs the reference stub, gymnasium's array Box, imports the reference)
import make_golden_ttc as mgt  # noqa: E402
import make_golden_lookahead as mgl  # noqa: E402
from oracle import ref_stub  # noqa: E402

from highway_env.envs.highway_env import HighwayEnvFast  # noqa: E402

GAMMA = 0.9
K_STEPS = 3


def continuous(**kw) -> dict:
    return dict({"type": "ContinuousAction"}, **kw)


SMALL = {"vehicles_count": 5, "lanes_count": 3, "duration": 30}
SCENARIOS = [
    # dense traffic, a wide steering range: some but not all sequences crash within their K steps
    dict(name="cem_crash", config=dict(SMALL, vehicles_count=12, vehicles_density=2.0, ego_spacing=1.0, action=continuous(steering_range=[-0.2, 0.2])),
         seeds=[400, 401, 404], warm=2, action_seed=701, sequences=8, sequence_seed=801),
    # full throttle, straight, until the ego runs into its leader: the parent is a finished episode at the branch point
    dict(name="cem_respawn", config=dict(SMALL, vehicles_count=10, vehicles_density=2.0, ego_spacing=1.0, action=continuous()),
         seeds=[0, 1, 2], until_crash=[1.25, 0.0], sequences=5, sequence_seed=802),
    # two agents
    dict(name="cem_ma2", config=dict(SMALL, vehicles_count=8, controlled_vehicles=2,
                                     observation={"type": "MultiAgentObservation", "observation_config": {"type": "Kinematics"}},
                                     action={"type": "MultiAgentAction", "action_config": continuous(steering_range=[-0.05, 0.05])}),
         seeds=[19, 20], warm=2, action_seed=703, sequences=5, sequence_seed=803),
    # one controlled axis: the action has one component
    dict(name="cem_longi_only", config=dict(SMALL, action=continuous(lateral=False)),
         seeds=[13, 14, 15], warm=2, action_seed=704, sequences=5, sequence_seed=804),
]
NAMES = [sc["name"] for sc in SCENARIOS]


def action_size(sc: dict) -> int:
    act = sc["config"]["action"]
    act = act.get("action_config", act)
    return int(act.get("longitudinal", True)) + int(act.get("lateral", True))


def as_action(a: np.ndarray, A: int):
    """float32 [A, size] -> what env.step takes."""
    return tuple(a[k].copy() for k in range(A)) if A > 1 else a[0].copy()


def run(sc: dict) -> dict:
    ref_stub.restore_class_defaults()
    seeds = sc["seeds"]
    A, size = int(sc["config"].get("controlled_vehicles", 1)), action_size(sc)
    B = sc["sequences"]
    seq = np.random.default_rng(sc["sequence_seed"]).uniform(-1.3, 1.3, size=(B, K_STEPS, A, size)).astype(np.float32)
    if "until_crash" in sc:
        warm_actions = None
    else:
        warm_actions = np.random.default_rng(sc["action_seed"]).uniform(-1.3, 1.3, size=(sc["warm"], len(seeds), A, size)).astype(np.float32)
    out = {"seeds": np.asarray(seeds, np.int64), "sequences": seq, "gamma": np.float64(GAMMA)}
    recs = []
    for e, seed in enumerate(seeds):
        env = HighwayEnvFast(dict(sc["config"]))
        env.reset(seed=int(seed))
        prev, prev_time, last, done, warm = None, 0.0, None, False, 0
        while True:
            if warm_actions is None:
                a = np.broadcast_to(np.asarray(sc["until_crash"], np.float32)[:size], (A, size)).copy()
            else:
                a = warm_actions[warm, e]
            prev, prev_time, last = mgc.dump_state(env), float(env.time), a.copy()
            _, _, term, trunc, _ = env.step(as_action(a, A))
            warm += 1
            done = bool(term or trunc)
            if (warm_actions is None and term) or (warm_actions is not None and warm == sc["warm"]):
                break
            assert warm < 40, f"{sc['name']} env {e}: no crash within 40 steps"
        rec = {"init": mgc.dump_state(env), "prev": prev, "prev_time": prev_time, "last": last, "done": done, "warm": warm,
               "behavior": mgt.behavior_of(env), "time": float(env.time), "cfg": dict(env.config),
               "T": int(env.config["simulation_frequency"] // env.config["policy_frequency"]),
               "reward": np.zeros((B, K_STEPS)), "terminated": np.zeros((B, K_STEPS), bool), "truncated": np.zeros((B, K_STEPS), bool),
               "crashed": np.zeros(B, bool)}
        for b in range(B):
            twin = copy.deepcopy(env)
            for k in range(K_STEPS):
                _, r, term, trunc, _ = twin.step(as_action(seq[b, k], A))
                rec["reward"][b, k], rec["terminated"][b, k], rec["truncated"][b, k] = r, term, trunc
            rec["crashed"][b] = twin.vehicle.crashed
        after = mgc.dump_state(env)
        assert all(np.array_equal(after[k], rec["init"][k], equal_nan=True) for k in after) and float(env.time) == rec["time"], \
            f"{sc['name']} env {e}: the parent changed under its copies"
        recs.append(rec)
    E = len(recs)
    out["meta"] = np.asarray([E, len(recs[0]["init"]["x"]), recs[0]["T"], max(r["warm"] for r in recs), 0], np.int64)
    mgt.config_record(out, recs[0]["cfg"], HighwayEnvFast, A, mgt.HORIZON)
    out["actions"] = np.zeros((0, E), np.int32)  # (the warm-up is not replayed: prev_* / last_action carry its last step)
    out["init_behavior"] = np.stack([r["behavior"] for r in recs])
    out["branch_time"] = np.asarray([r["time"] for r in recs], np.float64)
    out["prev_time"] = np.asarray([r["prev_time"] for r in recs], np.float64)
    out["last_action"] = np.stack([r["last"] for r in recs]).astype(np.float32)
    out["parent_done"] = np.asarray([r["done"] for r in recs], bool)
    for k in mgc.F64_FIELDS + mgc.I8_FIELDS:
        out["init_" + k] = np.stack([r["init"][k] for r in recs])
        out["prev_" + k] = np.stack([r["prev"][k] for r in recs])
    for k in ("reward", "terminated", "truncated", "crashed"):
        out[k] = np.stack([r[k] for r in recs])
    out["returns"] = np.array([[mgl.discounted(r["reward"][b], r["terminated"][b], r["truncated"][b], GAMMA) for b in range(B)] for r in recs])
    return out


def main() -> None:
    only = set(sys.argv[1:])
    mpath = os.path.join(HERE, "MANIFEST.json")
    manifest = json.load(open(mpath)) if os.path.exists(mpath) else {}
    for sc in SCENARIOS:
        if only and sc["name"] not in only:
            continue
        data = run(sc)
        if sc["name"] == "cem_crash":  # a crash INSIDE a sequence, and not in all of them
            c = data["crashed"].sum(axis=1)
            assert ((c > 0) & (c < data["crashed"].shape[1])).any() and not data["parent_done"].any(), c
            assert (data["terminated"].any(axis=2) & ~data["terminated"][:, :, 0]).any(), "no branch ends after its first step"
        if sc["name"] == "cem_respawn":
            assert data["parent_done"].all()
        path = os.path.join(HERE, sc["name"] + ".npz")
        np.savez_compressed(path, **data)
        with np.load(path) as z:
            manifest[sc["name"]] = mgc.digest(z)
        print(f"{sc['name']}: E,N,T,warm={data['meta'][:4].tolist()} B={data['sequences'].shape[0]} crashed branches per env "
              f"{data['crashed'].sum(axis=1).tolist()} parent done {data['parent_done'].tolist()} terminated "
              f"{int(data['terminated'].any(axis=2).sum())} -> {os.path.getsize(path) / 1024:.0f} KiB")
    with open(mpath, "w") as fh:
        json.dump(dict(sorted(manifest.items())), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
