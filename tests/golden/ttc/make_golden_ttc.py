#!/usr/bin/env python3
"""Generate the time-to-collision grid / finite-MDP fixtures in this directory from the UNMODIFIED reference.

TEST INFRASTRUCTURE.  Needs the reference package (``HWY_REFERENCE_ROOT``), imported through ``oracle/ref_stub.py`` like the
other generators:

    python tests/golden/ttc/make_golden_ttc.py [fixture ...]

The reference's ``AbstractEnv.to_finite_mdp()`` hands its tables to ``finite_mdp.mdp.DeterministicMDP``; an in-memory stand-in for
that module (it only keeps what it is given) is put into ``sys.modules``, so the call returns the reference's own tables.

Each fixture records a ``HighwayEnv`` / ``HighwayEnvFast`` run: the state at reset and after every step
(tests/golden/control/make_golden_control.py's record of a vehicle), the reference's ``compute_ttc_grid`` for every controlled
vehicle (``grid0`` [E, A, V, L, T], ``grid`` [steps, E, A, V, L, T]) and -- single-agent fixtures -- the tables of
``to_finite_mdp()``: ``transition0`` / ``transition`` (int32 [.., E, S, 5]), ``reward0`` / ``reward`` (f64), ``terminal0`` /
``terminal`` (bool [.., E, S]) and ``state0`` / ``state``.  (With ``MultiAgentAction`` the reference's ``env.action_space.n`` does
not exist, so ``to_finite_mdp()`` cannot run there; the grids of both agents are recorded.)

``ttc_crafted`` is not a run: every environment is a hand-placed road (CRAFTED below) written onto the vehicles of a reference
environment; ``steps`` is 0.  ``ttc_passes65`` / ``ttc_passes130`` are hand-placed too (PASS_SLOTS): vehicles within the horizon in
the slots either side of the kernel's passes of 64.  README.md says what each road is for.

No fixture holds a knife edge: for every candidate (other vehicle, ego speed, collision point) with q = ttc / tq < T + 1 the
generator asserts |q - rint(q)| >= 1e-9 (tests/ttc_util.py: restate_grid), except on the crafted roads whose headings are all
exactly 0, where the arithmetic is exact and the exact multiples are the point.  The digests of the arrays go to
``MANIFEST.json`` here.
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(GOLDEN, "control"))

import make_golden_control as mgc  # noqa: E402  (installs the reference stub, gymnasium's array Box, imports the reference)
from oracle import ref_stub  # noqa: E402

from highway_env.envs.common.finite_mdp import compute_ttc_grid  # noqa: E402
from highway_env.envs.highway_env import HighwayEnv, HighwayEnvFast  # noqa: E402
from highway_env.vehicle.behavior import LinearVehicle  # noqa: E402

LINEAR = "highway_env.vehicle.behavior.LinearVehicle"
HORIZON = 10.0  # finite_mdp(env, time_quantization, horizon=10.0): to_finite_mdp() leaves it at its default


class _DeterministicMDP:
    """Stand-in for finite_mdp.mdp.DeterministicMDP: keeps the tables finite_mdp() built."""

    def __init__(self, transition, reward, terminal=None, state=0):
        self.transition, self.reward, self.terminal, self.state = transition, reward, terminal, state


def install_finite_mdp_stub() -> None:
    if "finite_mdp.mdp" in sys.modules:
        return
    pkg, mod = types.ModuleType("finite_mdp"), types.ModuleType("finite_mdp.mdp")
    mod.DeterministicMDP = _DeterministicMDP
    pkg.mdp = mod
    sys.modules["finite_mdp"], sys.modules["finite_mdp.mdp"] = pkg, mod


install_finite_mdp_stub()

MA = {"observation": {"type": "MultiAgentObservation", "observation_config": {"type": "Kinematics"}},
      "action": {"type": "MultiAgentAction", "action_config": {"type": "DiscreteMetaAction"}}}
DENSE = {"vehicles_count": 30, "vehicles_density": 2.0, "lanes_count": 3, "ego_spacing": 1.0, "duration": 20}

BOUNDARY = {"vehicles_count": 30, "vehicles_density": 2.0, "ego_spacing": 1.0, "duration": 20, "lane_change_reward": -0.05,
            "right_lane_reward": 0.3}


def speeds(n: int) -> dict:
    """`n` target speeds from 16 m/s in steps of 3."""
    return {"type": "DiscreteMetaAction", "target_speeds": [16.0 + 3.0 * k for k in range(n)]}


SCENARIOS = [
    # highway-fast-v0 as it comes: 20 vehicles, 3 lanes, grid (3, 3, 10)
    dict(name="ttc_fast", cls=HighwayEnvFast, config={}, seeds=[0, 1, 2, 3], steps=6, action_seed=401),
    # one lane: max(L - 1, 1)
    dict(name="ttc_lanes1", cls=HighwayEnvFast, config={"lanes_count": 1, "vehicles_count": 10}, seeds=[4, 5], steps=3, action_seed=402),
    # sixteen lanes: every bit of the packed lane index
    dict(name="ttc_lanes16", cls=HighwayEnvFast, config={"lanes_count": 16, "vehicles_count": 60}, seeds=[6, 7], steps=3, action_seed=403),
    # 2 and 8 target speeds
    dict(name="ttc_speeds2", cls=HighwayEnvFast, config={"action": {"type": "DiscreteMetaAction", "target_speeds": [18.0, 28.0]}},
         seeds=[8, 9], steps=4, action_seed=404),
    dict(name="ttc_speeds8", cls=HighwayEnvFast,
         config={"lanes_count": 4, "action": {"type": "DiscreteMetaAction", "target_speeds": [12.0, 15.0, 18.0, 21.0, 24.0, 27.0, 30.0, 33.0]}},
         seeds=[10, 11], steps=4, action_seed=405),
    # policy_frequency 5: time step 0.2 s, T = 50 (highway-v0, 4 lanes: grid (3, 4, 50))
    dict(name="ttc_pf5", cls=HighwayEnv, config={"policy_frequency": 5, "vehicles_count": 30}, seeds=[12, 13], steps=4, action_seed=406),
    # horizon 1 s: T = 1, every state is terminal
    dict(name="ttc_horizon1", cls=HighwayEnvFast, config={}, seeds=[14, 15], steps=2, action_seed=407, horizon=1.0),
    # the passes of 64 vehicles: N = 64, 65, 130 (130: the workgroup step kernel's engine)
    dict(name="ttc_n64", cls=HighwayEnvFast, config={"vehicles_count": 63, "lanes_count": 4}, seeds=[16, 17], steps=2, action_seed=408),
    dict(name="ttc_n65", cls=HighwayEnvFast, config={"vehicles_count": 64, "lanes_count": 4}, seeds=[18, 19], steps=2, action_seed=409),
    dict(name="ttc_n130", cls=HighwayEnvFast, config={"vehicles_count": 129, "lanes_count": 4}, seeds=[20, 21], steps=2, action_seed=410),
    # two agents: the second as observer, the other agent as an obstacle
    dict(name="ttc_ma2", cls=HighwayEnvFast,
         config=dict(MA, vehicles_count=12, lanes_count=3, controlled_vehicles=2, ego_spacing=1.0, vehicles_density=2.0),
         seeds=[22, 23, 24], steps=5, action_seed=411),
    # LinearVehicle traffic
    dict(name="ttc_linear", cls=HighwayEnvFast, config={"vehicles_count": 30, "lanes_count": 4, "other_vehicles_type": LINEAR},
         seeds=[25, 26], steps=5, action_seed=412),
    # crash-rich: dense traffic at 15 Hz, crashed vehicles slowing down next to the observer
    dict(name="ttc_crash", cls=HighwayEnv, config=dict(DENSE), seeds=list(range(500, 508)), steps=6, action_seed=413),
    # non-zero lane_change_reward, another right_lane_reward
    dict(name="ttc_rewards", cls=HighwayEnvFast,
         config={"lane_change_reward": -0.05, "right_lane_reward": 0.3, "collision_reward": -2.5, "high_speed_reward": 0.7},
         seeds=[27, 28], steps=4, action_seed=414),
    # ---- the kernel's own boundaries (csrc/hwy_ttc.h) ----
    # 1024 cells: the small LDS class exactly full (4 x 4 x 64, horizon 64 s at 1 Hz), last cell index 1023
    dict(name="ttc_cells1024", cls=HighwayEnvFast, config=dict(BOUNDARY, lanes_count=4, action=speeds(4)), seeds=[2, 3], steps=2,
         action_seed=415, horizon=64.0),
    # 1025 cells: the first grid of the large class (5 x 5 x 41, horizon 41 s at 1 Hz)
    dict(name="ttc_cells1025", cls=HighwayEnvFast, config=dict(BOUNDARY, lanes_count=5, action=speeds(5)), seeds=[32, 33], steps=2,
         action_seed=416, horizon=41.0),
    # 64 states (4 x 16): one full pass of the value sweep and no second
    dict(name="ttc_states64", cls=HighwayEnvFast, config=dict(BOUNDARY, lanes_count=16, action=speeds(4)), seeds=[34, 35], steps=2,
         action_seed=417),
    # 65 states (5 x 13): a second pass with a tail of one thread, in the small class; and the hand-placed roads of STATE_ROADS
    dict(name="ttc_states65", cls=HighwayEnvFast, config=dict(BOUNDARY, lanes_count=13, action=speeds(5)), seeds=[36, 37], steps=2,
         action_seed=418, roads="ttc_states65"),
    # 8 x 16 x 64 = 8192 cells, 128 states (horizon 6.4 s at 10 Hz): every limit at once; grids and states only (the tables of
    # 8192 states do not fit the size of a committed fixture); and the hand-placed roads of STATE_ROADS
    dict(name="ttc_max", cls=HighwayEnvFast,
         config=dict(BOUNDARY, lanes_count=16, action=speeds(8), simulation_frequency=10, policy_frequency=10), seeds=[38, 39],
         steps=2, action_seed=419, horizon=6.4, roads="ttc_max", tables=False),
]

# ---- ttc_crafted: hand-placed roads ----------------------------------------------------------------------------------------------
# highway-fast-v0 with 4 lanes, target speeds [20, 25, 30], time step 1 s, T = 10.  Slot 0 is the observer at x = 100 on lane 1,
# heading 0, 25 m/s, speed index 1; each other vehicle is (x, lane, heading, speed); the slots a road does not use stand far away.
OBSERVER = (100.0, 1, 0.0, 25.0)
CRAFTED = [
    # 0  other.speed exactly a target speed (25): skipped for that ego speed only
    [(130.0, 1, 0.0, 25.0)],
    # 1  closing speed +0.005 / -0.005: utils.not_zero's two branches (0.053 / 0.01 = 5.3 cells; -0.043 / -0.01 = 4.3)
    [(105.053, 1, 0.0, 24.995), (94.957, 2, 0.0, 25.005)],
    # 2  a faster vehicle behind
    [(70.0, 1, 0.0, 29.0), (40.0, 0, 0.0, 33.5)],
    # 3  oncoming: heading pi
    [(307.0, 1, float(np.pi), 20.0), (423.0, 3, float(np.pi), 12.0)],
    # 4  exact multiples of the time step (headings exactly 0: 40 / 10 = 4, 40 / 5 = 8, 45 / 15 = 3): both quantisations, one cell
    [(140.0, 1, 0.0, 15.0)],
    # 5  ttc / tq exactly T = 10 for the centre point: out of range; the rear margin point (9.5) is in
    [(200.0, 2, 0.0, 15.0)],
    # 6  headings of 0.3 rad and -0.3 rad
    [(130.0, 2, 0.3, 22.0), (75.0, 0, -0.3, 31.0)],
    # 7  level with the observer and overlapping it: distance 0 (time 0 for every closing speed), the margins either side
    [(100.0, 2, 0.0, 21.0), (101.5, 1, 0.0, 27.0)],
    # 8  the observer turned by 0.2 rad: vehicle.direction enters the projected speed
    [(150.0, 1, 0.0, 18.0), (60.0, 3, 0.1, 32.0)],
    # 9  nothing within the horizon
    [],
    # 10 other.speed exactly a target speed (25), 37 mm ahead in the next lane: WITHOUT the `ego_speed == other.speed` skip
    #    utils.not_zero(0) = 0.01 puts the centre point at 3.7 s (on road 0 that time is 3000 s: beyond any horizon either way)
    [(100.037, 2, 0.0, 25.0)],
]
CRAFTED_OBSERVER_HEADING = {8: 0.2}
CRAFTED_SLOTS = 6
EXACT_ROADS = (0, 4, 5, 7)  # headings exactly 0 and candidates ON a cell boundary by construction

# ---- ttc_passes65 / ttc_passes130: the passes of 64 vehicles --------------------------------------------------------------------
# The same road and observer with N = 65 and N = 130 slots.  On a spawned road the slots from 64 on stand more than a kilometre
# ahead and mark nothing; here the vehicles within the horizon sit in the LAST slot of the first pass (63), the first slots of the
# second (64, 65), its last (127) and the first and the last slot of the third (128, 129 -- the tail), every one marking cells
# that no other vehicle marks (tests/test_ttc_host.py takes them away one by one).  Road 1 is road 0 moved and slowed a little.
PASS_SLOTS = {63: (131.7, 0, 0.0, 21.3), 64: (153.3, 1, 0.0, 17.9), 65: (78.1, 2, 0.0, 31.4),
              127: (168.9, 2, 0.0, 22.6), 128: (118.3, 0, 0.0, 16.2), 129: (139.4, 3, 0.0, 13.6)}
PASSES = {"ttc_passes65": 65, "ttc_passes130": 130}


# ---- ttc_states65 / ttc_max: the observer in the second pass of the value sweep ----------------------------------------------------
# The sweep gives thread `lane` the states s = h * L + i = lane and lane + 64.  On a spawned road the observer starts in the first
# pass; these roads -- further environments of the two runs, after the spawned ones -- put it on s = 63 (the last state of the
# first pass, whose RIGHT / FASTER neighbours lie in the second), 64 (the first of the second) and the last state.  Each road is
# (observer (x, lane, heading, speed, speed index), {slot: (x, lane, heading, speed)}): one vehicle ahead in the observer's lane,
# (`gap` m away: no crash within the recorded steps), which makes the five Q values differ, one in a neighbouring lane whose state lies in the second pass, one behind.
def _state_road(L: int, s: int, speeds_: list, gap: float, dx: float):
    h, i = divmod(s, L)
    side = i - 1 if i == L - 1 else i + 1          # a lane next to the observer's whose state h * L + side ...
    if h * L + side < 64:                          # ... lies in the second pass (s = 63: the one reached by FASTER instead)
        side = i
    ego = speeds_[h]
    return ((100.0, i, 0.0, ego, h),
            {1: (100.0 + gap + dx, i, 0.0, ego - 4.713), 2: (100.0 + 17.9 + dx, side, 0.0, ego - 2.917 + 3.0 * (side == i)),
             3: (100.0 - 9.1 - dx, max(i - 1, 0), 0.0, ego + 3.331)})


STATE_ROADS = {
    "ttc_states65": [_state_road(13, s, [16.0 + 3.0 * k for k in range(5)], 31.3, 0.37 * n) for n, s in enumerate((63, 64))],
    "ttc_max": [_state_road(16, s, [16.0 + 3.0 * k for k in range(8)], 21.3, 0.37 * n) for n, s in enumerate((63, 64, 127))],
}


def place(env, placed) -> None:
    """Write (x, lane, heading, speed) onto the vehicles of a reference environment, in list order."""
    for v, (x, lane, h, s) in zip(env.road.vehicles, placed):
        v.position = np.array([x, 4.0 * lane])
        v.heading, v.speed = h, s
        v.lane_index = ("0", "1", lane)
        v.lane = env.road.network.get_lane(v.lane_index)
        if hasattr(v, "target_lane_index"):
            v.target_lane_index = v.lane_index


def crafted_roads(name: str):
    """(slots, [{slot: (x, lane, heading, speed)}, ...]) of a hand-placed fixture."""
    if name == "ttc_crafted":
        return CRAFTED_SLOTS, [{1 + k: veh for k, veh in enumerate(road)} for road in CRAFTED]
    slots = PASSES[name]
    road0 = {k: veh for k, veh in PASS_SLOTS.items() if k < slots}
    road1 = {k: (x + 2.3, lane, h, s - 0.7) for k, (x, lane, h, s) in road0.items()}
    return slots, [road0, road1]


def behavior_of(env) -> np.ndarray:
    out = np.zeros((len(env.road.vehicles), 5))
    for i, v in enumerate(env.road.vehicles):
        if isinstance(v, LinearVehicle):
            out[i, :3], out[i, 3:] = v.ACCELERATION_PARAMETERS, v.STEERING_PARAMETERS
    return out


def config_record(out: dict, cfg: dict, cls, A: int, horizon: float) -> None:
    for k in ("lanes_count", "vehicles_count", "simulation_frequency", "policy_frequency", "normalize_reward", "offroad_terminal"):
        out["cfg_" + k] = np.int64(cfg[k])
    for k in ("duration", "ego_spacing", "vehicles_density", "collision_reward", "right_lane_reward", "high_speed_reward",
              "lane_change_reward"):
        out["cfg_" + k] = np.float64(cfg[k])
    out["cfg_reward_speed_range"] = np.asarray(cfg["reward_speed_range"], np.float64)
    out["cfg_fast"] = np.int64(cls is HighwayEnvFast)
    out["cfg_controlled_vehicles"] = np.int64(A)
    out["cfg_other_vehicles_type"] = np.asarray(cfg["other_vehicles_type"])
    out["cfg_observation_json"] = np.asarray(json.dumps(cfg["observation"]))
    out["cfg_action_json"] = np.asarray(json.dumps(cfg["action"]))
    out["cfg_horizon"] = np.float64(horizon)


def planning_record(env, A: int, horizon: float, tables: bool = True) -> dict:
    """The reference's grid of every controlled vehicle and, single agent, the tables of to_finite_mdp() (horizon 10) or of
    finite_mdp(env, 1 / policy_frequency, horizon) -- the same call with another horizon."""
    from highway_env.envs.common.finite_mdp import finite_mdp
    tq = 1 / env.config["policy_frequency"]
    rec = {"grid": np.stack([compute_ttc_grid(env, tq, horizon, vehicle=v) for v in env.controlled_vehicles])}
    if A == 1 and tables:
        mdp = env.to_finite_mdp() if horizon == HORIZON else finite_mdp(env, time_quantization=tq, horizon=horizon)
        assert mdp.original_shape == rec["grid"].shape[1:]
        rec.update(transition=np.asarray(mdp.transition, np.int32), reward=np.asarray(mdp.reward, np.float64),
                   terminal=np.asarray(mdp.terminal, bool), state=np.int64(mdp.state))
        assert rec["reward"].shape == rec["transition"].shape == (rec["grid"][0].size, 5)
    return rec


def assert_no_knife_edge(out: dict, name: str, exact_envs=()) -> float:
    """Every candidate of every recorded state keeps 1e-9 from a cell boundary (except the environments of `exact_envs`)."""
    from highwayenv_amd import _abi
    from tests import ttc_util
    g = ttc_util.TtcGolden(name, out)
    cfg, params = g.hwy_config(), g.params()
    closest = np.inf
    for index in g.indices():
        st = g.state("init" if index is None else "step", index)
        grid, edge, count, _ = ttc_util.restate_grid(cfg, st, params)
        np.testing.assert_array_equal(grid, g.get("grid", index), err_msg=f"{name}: the restatement disagrees with the reference")
        for e in range(g.E):
            if e in exact_envs:
                assert not st["heading"][e].any(), (name, e)
                continue
            one = _abi.make_config(g.config, 1, fast=g.fast)
            _, edge1, _, c = ttc_util.restate_grid(one, {k: v[e:e + 1] for k, v in st.items()}, params)
            assert not edge1.any() and c >= ttc_util.KNIFE, f"{name} env {e} state {index}: a candidate {c} from a cell boundary"
            closest = min(closest, c)
    return closest


def run(sc: dict, only_envs=None) -> dict:
    """`only_envs`: simulate only these env indices (the actions are drawn for all of them either way)."""
    ref_stub.restore_class_defaults()
    seeds, steps = sc["seeds"], sc["steps"]
    horizon = float(sc.get("horizon", HORIZON))
    A = int(sc["config"].get("controlled_vehicles", 1))
    roads = STATE_ROADS[sc["roads"]] if "roads" in sc else []   # hand-placed environments after the spawned ones (seed 0)
    tables = sc.get("tables", True)
    seeds = list(seeds) + [0] * len(roads)
    actions = np.random.default_rng(sc["action_seed"]).integers(0, 5, size=(steps, len(seeds), A)).astype(np.int32)
    out = {"seeds": np.asarray(seeds, np.int64), "actions": actions}
    recs = []
    for e, seed in enumerate(seeds):
        if only_envs is not None and e not in only_envs:
            continue
        env = sc["cls"](dict(sc["config"]))
        env.reset(seed=int(seed))
        if e >= len(seeds) - len(roads):
            (x, lane, h, s, index), others = roads[e - (len(seeds) - len(roads))]
            n, last = len(env.road.vehicles), sc["config"]["lanes_count"] - 1
            assert env.road.vehicles[0] is env.vehicle and 0 not in others and max(others) < n
            place(env, [(x, lane, h, s) if k == 0 else others.get(k, (6000.0 + 150.0 * k, last, 0.0, 20.0)) for k in range(n)])
            env.vehicle.speed_index, env.vehicle.target_speed = index, env.vehicle.index_to_speed(index)
        rec = {"init": mgc.dump_state(env), "behavior": behavior_of(env), "plan0": planning_record(env, A, horizon, tables),
               "plan": [], "step_state": []}
        for t in range(steps):
            env.step(tuple(int(v) for v in actions[t, e]) if A > 1 else int(actions[t, e, 0]))
            rec["step_state"].append(mgc.dump_state(env))
            rec["plan"].append(planning_record(env, A, horizon, tables))
        rec["T"] = int(env.config["simulation_frequency"] // env.config["policy_frequency"])
        rec["cfg"] = dict(env.config)
        recs.append(rec)
    out["meta"] = np.asarray([len(recs), len(recs[0]["init"]["x"]), recs[0]["T"], steps, 0], np.int64)
    config_record(out, recs[0]["cfg"], sc["cls"], A, horizon)
    out["init_behavior"] = np.stack([r["behavior"] for r in recs])
    for k in recs[0]["plan0"]:
        out[k + "0"] = np.stack([r["plan0"][k] for r in recs])                                       # [E, ...]
        out[k] = np.stack([np.stack([p[k] for p in r["plan"]]) for r in recs], axis=1)               # [steps, E, ...]
    for k in mgc.F64_FIELDS + mgc.I8_FIELDS:
        out["init_" + k] = np.stack([r["init"][k] for r in recs])
        out["step_" + k] = np.stack([np.stack([s[k] for s in r["step_state"]]) for r in recs], axis=1)
    return out


def run_crafted(name: str = "ttc_crafted", only_envs=None) -> dict:
    ref_stub.restore_class_defaults()
    slots, roads = crafted_roads(name)
    headings = CRAFTED_OBSERVER_HEADING if name == "ttc_crafted" else {}
    config = {"vehicles_count": slots - 1, "lanes_count": 4}
    recs = []
    for e, road in enumerate(roads):
        if only_envs is not None and e not in only_envs:
            continue
        env = HighwayEnvFast(dict(config))
        env.reset(seed=0)
        assert len(env.road.vehicles) == slots and env.road.vehicles[0] is env.vehicle and 0 not in road and max(road, default=0) < slots
        placed = {0: OBSERVER[:2] + (headings.get(e, 0.0), OBSERVER[3]), **road}
        far = iter((6000.0 + 150.0 * k, 3, 0.0, 20.0) for k in range(slots))  # the slots a road does not use
        placed = [placed[k] if k in placed else next(far) for k in range(slots)]
        place(env, placed)
        env.vehicle.speed_index, env.vehicle.target_speed = 1, 25.0
        recs.append({"init": mgc.dump_state(env), "plan0": planning_record(env, 1, HORIZON), "cfg": dict(env.config)})
    out = {"seeds": np.zeros(len(roads), np.int64), "actions": np.zeros((0, len(roads), 1), np.int32)}
    out["meta"] = np.asarray([len(recs), slots, 5, 0, 0], np.int64)
    config_record(out, recs[0]["cfg"], HighwayEnvFast, 1, HORIZON)
    out["init_behavior"] = np.zeros((len(recs), slots, 5))
    for k in recs[0]["plan0"]:
        out[k + "0"] = np.stack([r["plan0"][k] for r in recs])
    for k in mgc.F64_FIELDS + mgc.I8_FIELDS:
        out["init_" + k] = np.stack([r["init"][k] for r in recs])
    return out


HAND_PLACED = ["ttc_crafted"] + list(PASSES)
NAMES = [sc["name"] for sc in SCENARIOS] + HAND_PLACED


def generate(name: str, only_envs=None) -> dict:
    if name in HAND_PLACED:
        return run_crafted(name, only_envs)
    return run(next(sc for sc in SCENARIOS if sc["name"] == name), only_envs)


def main() -> None:
    only = set(sys.argv[1:])
    mpath = os.path.join(HERE, "MANIFEST.json")
    manifest = json.load(open(mpath)) if os.path.exists(mpath) else {}
    for name in NAMES:
        if only and name not in only:
            continue
        data = generate(name)
        closest = assert_no_knife_edge(data, name, exact_envs=EXACT_ROADS if name == "ttc_crafted" else ())
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **data)
        with np.load(path) as z:
            manifest[name] = mgc.digest(z)
        print(f"{name}: E,N,T,steps={data['meta'][:4].tolist()} grid {data['grid0'].shape[1:]} marked cells at reset "
              f"{(data['grid0'] > 0).mean():.3f} closest candidate to a boundary {closest:.3g} -> {os.path.getsize(path) / 1024:.0f} KiB")
    with open(mpath, "w") as fh:
        json.dump(dict(sorted(manifest.items())), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
