"""Fixtures of the simulator-based planning seam, recorded from the UNMODIFIED reference: ``copy.deepcopy(env)`` followed by
``env.step`` on the copy (AbstractEnv.__deepcopy__, envs/common/abstract.py:455; scripts/highway_planning.ipynb).

TEST INFRASTRUCTURE.  Needs the reference package (``HWY_REFERENCE_ROOT``), imported through ``oracle/ref_stub.py`` like the
other generators (tests/golden/control/make_golden_control.py installs the stub and records a vehicle; tests/golden/ttc's
generator supplies the config record).  Per environment of a fixture: ``reset(seed)``, a few recorded warm-up steps, the state at
the branch point (``init_*``, ``init_behavior``, ``branch_time``), and then for EVERY candidate sequence a deep copy of the
environment stepped K times: ``reward`` / ``terminated`` / ``truncated`` [E, B, K] (several agents: the reference's reward is its
first controlled vehicle's) and the discounted ``returns`` [E, B] at ``gamma`` by the recurrence of include/hwy_engine.h
(hwy_score_device) in Python floats, ``q`` [E, n_ids] and ``best_action`` [E] from them.  The parent is checked to be unchanged by
its copies.  Single-agent meta-action fixtures hold the 25 depth-2 sequences padded to K = 4 with IDLE (``plan_lookahead(2, 4)``);
the two-agent and the DiscreteAction fixture hold explicit sequences drawn from ``sequence_seed``.

The generator asserts what lets the tests compare without exclusions: in every environment the two best entries of ``q`` are
either exactly equal (identical trajectories) or more than 1e-6 apart, and some fixture has some but not all branches crashing.

    HWY_REFERENCE_ROOT=... python tests/golden/lookahead/make_golden_lookahead.py [name ...]
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

import make_golden_control as mgc  # noqa: E402  (installs the reference stub, gymnasium's array Box, imports the reference)
import make_golden_ttc as mgt  # noqa: E402
from oracle import ref_stub  # noqa: E402

from highway_env.envs.highway_env import HighwayEnv, HighwayEnvFast  # noqa: E402

GAMMA = 0.9
K_STEPS = 4
GAP = 1e-6

SCENARIOS = [
    # highway-fast-v0 as it comes.  Seed 0 after 2 steps: 5 of 25 branches crash, IDLE and LANE_LEFT tie exactly on lane 0
    dict(name="la_fast", cls=HighwayEnvFast, config={}, seeds=[0, 1, 2], warm=2, action_seed=501),
    # every branch is truncated at step 2 of 4: time 2 s at the branch point, duration 4 s
    dict(name="la_trunc", cls=HighwayEnvFast, config={"duration": 4, "vehicles_count": 15}, seeds=[3, 4], warm=2, action_seed=502),
    # highway-v0: 15 frames per policy step, every pair checked for collisions
    dict(name="la_v0", cls=HighwayEnv, config={"vehicles_count": 20, "vehicles_density": 1.5}, seeds=[5, 6], warm=2, action_seed=503),
    # LinearVehicle traffic: the behaviour planes travel with the fork
    dict(name="la_linear", cls=HighwayEnvFast, config={"vehicles_count": 20, "other_vehicles_type": mgt.LINEAR}, seeds=[7, 8], warm=3,
         action_seed=504),
    # two agents, explicit [B, K, 2] sequences
    dict(name="la_ma2", cls=HighwayEnvFast,
         config=dict(mgt.MA, vehicles_count=12, lanes_count=3, controlled_vehicles=2, ego_spacing=1.0, vehicles_density=2.0),
         seeds=[9, 10], warm=2, action_seed=505, sequences=12, sequence_seed=605),
    # a DiscreteAction ego (throttle x steering, 3 x 3), explicit sequences: the stored controls travel with the fork
    dict(name="la_direct", cls=HighwayEnvFast, config={"vehicles_count": 15, "action": mgc.discrete(steering_range=[-0.1, 0.1])},
         seeds=[11, 12], warm=2, action_seed=506, sequences=12, sequence_seed=606),
]
NAMES = [sc["name"] for sc in SCENARIOS]


def num_ids(sc: dict) -> int:
    act = sc["config"].get("action", {})
    act = act.get("action_config", act)
    return int(act.get("actions_per_axis", 3)) ** 2 if act.get("type") == "DiscreteAction" else 5


def sequences_of(sc: dict, A: int) -> np.ndarray:
    """int32 [B, K, A]: the depth-2 tree padded with IDLE, or `sequences` random ones."""
    n = num_ids(sc)
    if "sequences" in sc:
        return np.random.default_rng(sc["sequence_seed"]).integers(0, n, size=(sc["sequences"], K_STEPS, A)).astype(np.int32)
    b = np.arange(n * n)
    table = np.full((b.size, K_STEPS, 1), 1, np.int32)  # IDLE
    table[:, 0, 0], table[:, 1, 0] = b // n, b % n
    return table


def discounted(reward, terminated, truncated, gamma: float) -> float:
    g, d, alive = 0.0, 1.0, True
    for k in range(len(reward)):
        if alive:
            t = d * float(reward[k])
            g = g + t
        alive = alive and not (terminated[k] or truncated[k])
        d = d * gamma
    return g


def run(sc: dict, only_envs=None) -> dict:
    ref_stub.restore_class_defaults()
    seeds, warm = sc["seeds"], sc["warm"]
    A = int(sc["config"].get("controlled_vehicles", 1))
    n = num_ids(sc)
    warm_actions = np.random.default_rng(sc["action_seed"]).integers(0, n, size=(warm, len(seeds), A)).astype(np.int32)
    seq = sequences_of(sc, A)
    B = seq.shape[0]
    out = {"seeds": np.asarray(seeds, np.int64), "actions": warm_actions, "sequences": seq, "gamma": np.float64(GAMMA)}
    recs = []
    for e, seed in enumerate(seeds):
        if only_envs is not None and e not in only_envs:
            continue
        env = sc["cls"](dict(sc["config"]))
        env.reset(seed=int(seed))
        for t in range(warm):
            env.step(tuple(int(v) for v in warm_actions[t, e]) if A > 1 else int(warm_actions[t, e, 0]))
        rec = {"init": mgc.dump_state(env), "behavior": mgt.behavior_of(env), "time": float(env.time), "cfg": dict(env.config),
               "T": int(env.config["simulation_frequency"] // env.config["policy_frequency"]),
               "reward": np.zeros((B, K_STEPS)), "terminated": np.zeros((B, K_STEPS), bool), "truncated": np.zeros((B, K_STEPS), bool),
               "crashed": np.zeros(B, bool)}
        for b in range(B):
            twin = copy.deepcopy(env)
            for k in range(K_STEPS):
                _, r, term, trunc, _ = twin.step(tuple(int(v) for v in seq[b, k]) if A > 1 else int(seq[b, k, 0]))
                rec["reward"][b, k], rec["terminated"][b, k], rec["truncated"][b, k] = r, term, trunc
            rec["crashed"][b] = twin.vehicle.crashed
        after = mgc.dump_state(env)
        assert all(np.array_equal(after[k], rec["init"][k], equal_nan=True) for k in after) and float(env.time) == rec["time"], \
            f"{sc['name']} env {e}: the parent changed under its copies"
        recs.append(rec)
    E = len(recs)
    out["meta"] = np.asarray([E, len(recs[0]["init"]["x"]), recs[0]["T"], warm, 0], np.int64)
    mgt.config_record(out, recs[0]["cfg"], sc["cls"], A, mgt.HORIZON)
    out["init_behavior"] = np.stack([r["behavior"] for r in recs])
    out["branch_time"] = np.asarray([r["time"] for r in recs], np.float64)
    for k in mgc.F64_FIELDS + mgc.I8_FIELDS:
        out["init_" + k] = np.stack([r["init"][k] for r in recs])
    for k in ("reward", "terminated", "truncated", "crashed"):
        out[k] = np.stack([r[k] for r in recs])
    ret = np.array([[discounted(r["reward"][b], r["terminated"][b], r["truncated"][b], GAMMA) for b in range(B)] for r in recs])
    out["returns"] = ret
    q = np.full((E, n), -np.inf)
    for b in range(B):  # the maximum over the branches that start with each action (agent 0's)
        q[:, seq[b, 0, 0]] = np.maximum(q[:, seq[b, 0, 0]], ret[:, b])
    out["q"], out["best_action"] = q, np.argmax(q, axis=1).astype(np.int32)
    return out


def assert_decidable(out: dict, name: str) -> float:
    """The two best first actions of every environment: exactly equal, or more than GAP apart.  Returns the smallest non-zero gap."""
    smallest = np.inf
    for e, row in enumerate(out["q"]):
        top = np.sort(row[np.isfinite(row)])[::-1]
        if top.size > 1:
            gap = top[0] - top[1]
            assert gap == 0 or gap > GAP, f"{name} env {e}: the two best first actions are {gap} apart"
            if gap > 0:
                smallest = min(smallest, gap)
    return smallest


def generate(name: str, only_envs=None) -> dict:
    return run(next(sc for sc in SCENARIOS if sc["name"] == name), only_envs)


def main() -> None:
    only = set(sys.argv[1:])
    mpath = os.path.join(HERE, "MANIFEST.json")
    manifest = json.load(open(mpath)) if os.path.exists(mpath) else {}
    for name in NAMES:
        if only and name not in only:
            continue
        data = generate(name)
        gap = assert_decidable(data, name)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **data)
        with np.load(path) as z:
            manifest[name] = mgc.digest(z)
        print(f"{name}: E,N,T,warm={data['meta'][:4].tolist()} B={data['sequences'].shape[0]} crashed branches per env "
              f"{data['crashed'].sum(axis=1).tolist()} truncated {int(data['truncated'].any(axis=2).sum())} terminated "
              f"{int(data['terminated'].any(axis=2).sum())} best {data['best_action'].tolist()} smallest gap {gap:.3g} -> "
              f"{os.path.getsize(path) / 1024:.0f} KiB")
    mixed = bool(only)  # (checked when the whole set is generated)
    for name in ([] if only else NAMES):  # some but not all branches of an environment crash, somewhere
        with np.load(os.path.join(HERE, name + ".npz")) as z:
            c = z["crashed"].sum(axis=1)
            mixed = mixed or bool(((c > 0) & (c < z["crashed"].shape[1])).any())
    assert mixed, "no fixture has an environment in which some but not all branches crash"
    with open(mpath, "w") as fh:
        json.dump(dict(sorted(manifest.items())), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
