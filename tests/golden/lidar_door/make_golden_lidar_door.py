#!/usr/bin/env python3
"""Generate the fixtures of the Lidar door (csrc/hwy_lidar_door.h) in this directory from the UNMODIFIED reference.

TEST INFRASTRUCTURE.  Needs the reference package (``HWY_REFERENCE_ROOT``), imported through ``oracle/ref_stub.py`` like the
other generators:

    python tests/golden/lidar_door/make_golden_lidar_door.py [fixture ...]

Every fixture records reference environments whose ``config["observation"]`` is a ``LidarObservation`` (several agents: under
``MultiAgentObservation``) in the record of the family's own generator -- tests/golden/make_golden_merge.py (``door_merge*``,
``door_crafted``: vehicles in list order, absent slots, the road objects at the END), tests/golden/make_golden_intersection.py
(``door_ix*``: the compact list after ``_clear_vehicles`` / ``_spawn_vehicle``, ``next_*``) and tests/golden/lidar/make_golden_lidar.py
(``door_cells``) -- so that tests/golden_util.py's loaders put a recorded state on an engine, and next to every state the
reference's observation of it:

* ``obs0`` [E, A, cells, 2] / ``obs`` [steps, E, A, cells, 2]: what ``reset()`` / ``step()`` returned;
* ``door_ix*``: also ``observe`` [steps, E, A, cells, 2], ``observation_type.observe()`` called AFTER ``step()`` -- the yardstick of
  these fixtures, since ``IntersectionEnv.step`` observes BEFORE it clears and spawns vehicles (intersection_env.py:136-140).  The
  generator asserts that at least one recorded step differs between the two and that the list shrinks or grows at least once;
* ``door_cells``: ``obs0_c<cells>`` / ``obs_c<cells>`` for cells = 1, 65 and 256: ``LidarObservation(env, cells=...)`` of the
  reference, constructed on the recorded environment and observed at reset and after every step (the reference has no cap).

``door_crafted`` is not a run: every environment is a hand-placed road (CRAFTED below) written onto the vehicles and the Obstacle of a
reference ``MergeEnv``; ``obs0`` is the reference's ``observe()`` of it and ``steps`` is 0.

The generator ASSERTS two conditions on every recorded state and refuses to write a fixture that breaks either (conditions on the
inputs, not tolerances): no candidate angle (centre or corner of a traced obstacle) lies within 1e-9 rad of a cell boundary, and no
centre distance lies within 1e-9 m of ``maximum_range``.  With one cell every angle maps to cell 0 and the first condition is
empty.  The crafted ties (TIE below) are equal DISTANCES, exact by construction; they are the only knife edges in here.
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
sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(GOLDEN, "control"))
sys.path.insert(0, os.path.join(GOLDEN, "lidar"))

import make_golden_control as mgc  # noqa: E402  (installs the reference stub, gymnasium's array Box, imports the reference)
import make_golden_intersection as mgi  # noqa: E402
import make_golden_lidar as mgl  # noqa: E402
import make_golden_merge as mgm  # noqa: E402
from oracle import ref_stub  # noqa: E402

from highway_env import utils  # noqa: E402
from highway_env.envs.common.observation import LidarObservation  # noqa: E402
from highway_env.envs.highway_env import HighwayEnvFast  # noqa: E402
from highway_env.envs.intersection_env import IntersectionEnv, MultiAgentIntersectionEnv  # noqa: E402
from highway_env.envs.merge_env import ConnectedLaneMergeEnv, MergeEnv  # noqa: E402

MARGIN = 1e-9
CELLS_EXTRA = (1, 65, 256)


def lidar(**kw) -> dict:
    return dict({"type": "LidarObservation"}, **kw)


def multi(obs: dict) -> dict:
    return {"observation": {"type": "MultiAgentObservation", "observation_config": obs},
            "action": {"type": "MultiAgentAction", "action_config": {"type": "DiscreteMetaAction"}}}


def lidar_of(config: dict) -> dict:
    obs = config["observation"]
    obs = obs.get("observation_config", obs)
    return {"cells": int(obs.get("cells", 16)), "maximum_range": float(obs.get("maximum_range", 60)), "normalize": bool(obs.get("normalize", True))}


# ---- the two conditions on the inputs ---------------------------------------------------------------------------------------------
def assert_margins(what: str, x, y, heading, present, controlled, obstacle, cells: int, maximum_range: float) -> tuple:
    """[..., N] planes of recorded states.  Returns the smallest angle and range margins met."""
    cell = 2 * np.pi / cells
    x, y, heading = (np.asarray(a, np.float64).reshape(-1, np.shape(x)[-1]) for a in (x, y, heading))
    present, controlled, obstacle = (np.asarray(a).reshape(x.shape) != 0 for a in (present, controlled, obstacle))
    min_angle, min_range = np.inf, np.inf
    for r in range(x.shape[0]):
        for me in np.nonzero(present[r] & controlled[r])[0]:
            origin = np.array([x[r, me], y[r, me]])
            for j in np.nonzero(present[r])[0]:
                if j == me:
                    continue
                pos = np.array([x[r, j], y[r, j]])
                d = np.linalg.norm(pos - origin)
                min_range = min(min_range, abs(d - maximum_range))
                if d > maximum_range or cells == 1:
                    continue
                corners = utils.rect_corners(pos, 2.0 if obstacle[r, j] else 5.0, 2.0, heading[r, j])
                for p in [pos] + list(corners):
                    q = (np.arctan2(p[1] - origin[1], p[0] - origin[0]) + cell / 2) / cell
                    min_angle = min(min_angle, abs(q - np.rint(q)) * cell)
    assert min_angle >= MARGIN, f"{what}: a candidate angle lies {min_angle:.3g} rad from a cell boundary"
    assert min_range >= MARGIN, f"{what}: a centre distance lies {min_range:.3g} m from maximum_range"
    return min_angle, min_range


def merge_margins(name: str, data: dict, prefixes, cells, maximum_range) -> tuple:
    out = [assert_margins(f"{name} {p}", data[p + "_x"], data[p + "_y"], data[p + "_heading"], data[p + "_present"], data[p + "_controlled"],
                          data[p + "_obstacle"] if p + "_obstacle" in data else np.zeros_like(data[p + "_present"]), cells, maximum_range)
           for p in prefixes]
    return min(o[0] for o in out), min(o[1] for o in out)


# ---- merge scenarios: tests/golden/make_golden_merge.py's record, with the Lidar observation as `obs0` / `obs` ------------------------------
MERGE = [
    # merge-v0 as it comes: the ramp vehicle on the SineLane with a heading that is not 0; the ego passes the Obstacle (x = 310)
    dict(name="door_merge", cls=MergeEnv, config={"observation": lidar()}, seeds=[0, 1, 2], steps=12, action_seed=601, frames_for=0, n_slots=6),
    # merge-generic with 4 controlled vehicles (BASELINE config 5's shape) and absent slots: raw values, 24 cells, 80 m
    dict(name="door_merge_generic_ma4", cls=mgm.MergeGenericMultiAgent,
         config=dict(multi(lidar(cells=24, maximum_range=80, normalize=False)), lanes_count=4, vehicles_count=40, controlled_vehicles=4),
         seeds=[0, 1], steps=6, action_seed=602, frames_for=0, n_slots=43),
    # the connected-lane variant
    dict(name="door_merge_v1", cls=ConnectedLaneMergeEnv, config={"observation": lidar(cells=32)}, seeds=[3, 4], steps=12, action_seed=603,
         frames_for=0, n_slots=6),
]


def run_merge(sc: dict) -> dict:
    data = mgm.run_scenario(sc)
    assert data["obs0"].dtype == np.float32 and data["obs"].dtype == np.float32
    p = lidar_of(sc["config"])
    data["lidar_json"] = np.asarray(json.dumps(p))
    data["margins"] = np.asarray(merge_margins(sc["name"], data, ("init", "step"), p["cells"], p["maximum_range"]))
    if sc["name"] == "door_merge":  # the Obstacle within range of the ego, and the ramp vehicle with a heading that is not 0
        obst = data["step_obstacle"] != 0
        d = np.hypot(data["step_x"] - data["step_x"][..., :1], data["step_y"] - data["step_y"][..., :1])
        assert (d[obst] < p["maximum_range"]).any(), "the Obstacle never comes within range"
        ramp = (np.abs(data["step_heading"][..., 4]) > 1e-2) & (d[..., 4] < p["maximum_range"])
        assert ramp.any(), "the ramp vehicle is never traced with a heading that is not 0"
    if sc["name"] == "door_merge_generic_ma4":
        assert (data["init_present"] == 0).any(), "no absent slot"
    return data


# ---- intersection: tests/golden/make_golden_intersection.py's record of the list AFTER clear / spawn --------------------------------------
IX = [
    # (vehicles are spawned 100 m from the centre of the junction and cleared near the ends of the arms: a range of 120 m sees them)
    dict(name="door_ix", cls=IntersectionEnv,
         config={"observation": lidar(maximum_range=120), "initial_vehicle_count": 12, "spawn_probability": 0.9},
         seeds=[0, 1, 2], steps=12, action_seed=611, n_slots=32),
    dict(name="door_ix_ma3", cls=MultiAgentIntersectionEnv,
         config=dict(observation=multi(lidar(cells=20, maximum_range=110, normalize=False))["observation"], controlled_vehicles=3,
                     initial_vehicle_count=10, spawn_probability=0.9),  # (the env's own longitudinal MultiAgentAction)
         seeds=[5, 6], steps=12, action_seed=612, n_slots=32),
]


def run_ix(sc: dict) -> dict:
    ref_stub.restore_class_defaults()
    seeds, steps, n_slots, cls = sc["seeds"], sc["steps"], sc["n_slots"], sc["cls"]
    is_multi = cls is MultiAgentIntersectionEnv
    A = int(dict(cls.default_config(), **sc["config"])["controlled_vehicles"])
    r_max = mgi.R_MAX_MA if is_multi else mgi.R_MAX
    actions = np.random.default_rng(sc["action_seed"]).integers(0, 3, size=(steps, len(seeds), A)).astype(np.int32)
    out = {"seeds": np.asarray(seeds, np.int64), "actions": actions}
    stack = lambda o: np.stack(o) if is_multi else np.asarray(o)[None]  # noqa: E731
    recs, tab0 = [], None
    for e, seed in enumerate(seeds):
        env = cls(dict(sc["config"]))
        obs0, _ = env.reset(seed=int(seed))
        tab, index, nodes = mgi.lane_table(env.road.network)
        tab0 = tab if tab0 is None else tab0
        vids: dict = {}
        rec = {"obs0": stack(obs0), "init": mgi.dump_state(env, index, nodes, n_slots, vids, r_max), "road_steps0": env.road.steps,
               "obs": [], "observe": [], "next": [], "road_steps": [], "terminated": [], "truncated": []}
        for t in range(steps):
            o, r, te, tr, info = env.step(tuple(int(a) for a in actions[t, e]) if is_multi else int(actions[t, e, 0]))
            rec["obs"].append(stack(o))
            rec["observe"].append(stack(env.observation_type.observe()))  # of the list after _clear_vehicles / _spawn_vehicle
            rec["next"].append(mgi.dump_state(env, index, nodes, n_slots, vids, r_max))
            rec["road_steps"].append(env.road.steps)
            rec["terminated"].append(te)
            rec["truncated"].append(tr)
        rec["T"] = int(env.config["simulation_frequency"] // env.config["policy_frequency"])
        rec["cfg"], rec["nodes"] = dict(env.config), nodes
        recs.append(rec)
    cfg = recs[0]["cfg"]
    out["meta"] = np.asarray([len(recs), n_slots, recs[0]["T"], steps, 0, A, r_max], np.int64)
    out["cfg_json"] = np.asarray(json.dumps({k: v for k, v in cfg.items() if isinstance(v, (int, float, str, bool, list, dict, type(None)))}))
    for k in mgi.LANE_F64 + mgi.LANE_I32:
        out["lane_" + k] = tab0[k]
    out["node_names"] = np.asarray(list(recs[0]["nodes"].keys()))
    out["road_steps0"] = np.asarray([r["road_steps0"] for r in recs], np.int64)
    out["next_road_steps"] = np.asarray([r["road_steps"] for r in recs], np.int64).T              # [steps, E]
    out["obs0"] = np.stack([r["obs0"] for r in recs])                                             # [E, A, cells, 2]
    out["obs"] = np.stack([np.stack(r["obs"]) for r in recs], axis=1)                             # [steps, E, A, cells, 2]
    out["observe"] = np.stack([np.stack(r["observe"]) for r in recs], axis=1)
    out["terminated"] = np.asarray([r["terminated"] for r in recs], np.int8).T
    out["truncated"] = np.asarray([r["truncated"] for r in recs], np.int8).T
    for k in mgi.F64_FIELDS + mgi.INT_FIELDS + mgi.ROUTE_FIELDS:
        out["init_" + k] = np.stack([r["init"][k] for r in recs])
        out["next_" + k] = np.stack([np.stack([s[k] for s in r["next"]]) for r in recs], axis=1)
    assert out["obs"].dtype == np.float32 and out["observe"].dtype == np.float32
    p = lidar_of(sc["config"])
    out["lidar_json"] = np.asarray(json.dumps(p))
    out["margins"] = np.asarray(merge_margins(sc["name"], out, ("init", "next"), p["cells"], p["maximum_range"]))
    # the documented reason why the vector env refuses the option here: step()'s observation is of the list BEFORE clear / spawn
    assert (np.abs(out["obs"] - out["observe"]).max(axis=(2, 3, 4)) > 1e-6).any(), "step() and observe() never differ"
    counts = np.concatenate([out["init_present"].sum(-1)[None], out["next_present"].sum(-1)])
    assert (np.diff(counts, axis=0) != 0).any(), "the list never shrinks or grows"
    return out


# ---- door_cells: highway-fast-v0, the reference's LidarObservation with 1, 65 and 256 cells on the same recorded run -------------------
CELLS = dict(name="door_cells", cls=HighwayEnvFast, config={"vehicles_count": 30, "lanes_count": 4, "observation": lidar(cells=65)},
             seeds=[0, 1], steps=5, action_seed=621)


def run_cells(sc: dict) -> dict:
    """make_golden_lidar.py's `run`, with the extra observers asked at reset and after every step."""
    extra = {c: {"obs0": [], "obs": []} for c in CELLS_EXTRA}
    step0 = HighwayEnvFast.step
    reset0 = HighwayEnvFast.reset

    def observers(env):
        return {c: LidarObservation(env, cells=c) for c in CELLS_EXTRA}

    def reset(self, **kw):
        out = reset0(self, **kw)
        for c, o in observers(self).items():
            if extra[c]["obs"] and not extra[c]["obs"][-1]:  # (AbstractEnv.__init__ resets once before the seeded reset)
                extra[c]["obs0"].pop()
                extra[c]["obs"].pop()
            extra[c]["obs0"].append(o.observe()[None])
            extra[c]["obs"].append([])
        return out

    def step(self, action):
        out = step0(self, action)
        for c, o in observers(self).items():
            extra[c]["obs"][-1].append(o.observe()[None])
        return out

    cls = type("Observed", (HighwayEnvFast,), {"reset": reset, "step": step})  # (a subclass: the reference's class is not touched)
    data = mgl.run(dict(sc, cls=cls))
    data["cfg_fast"] = np.int64(1)
    for c in CELLS_EXTRA:
        data[f"obs0_c{c}"] = np.stack(extra[c]["obs0"])                                        # [E, 1, c, 2]
        data[f"obs_c{c}"] = np.stack([np.stack(o) for o in extra[c]["obs"]], axis=1)           # [steps, E, 1, c, 2]
        assert data[f"obs_c{c}"].dtype == np.float32
    np.testing.assert_array_equal(data["obs_c65"], data["obs"])  # (the configured observer and the constructed one agree)
    ctrl, pres = data["init_controlled"], np.ones_like(data["init_controlled"])
    margins = []
    for c in CELLS_EXTRA:
        for p in ("init", "step"):
            shape = data[p + "_x"].shape
            margins.append(assert_margins(f"door_cells {p} cells={c}", data[p + "_x"], data[p + "_y"], data[p + "_heading"],
                                          np.broadcast_to(pres, shape), np.broadcast_to(ctrl, shape), np.zeros(shape), c, 60.0))
    data["margins"] = np.asarray([min(m[0] for m in margins), min(m[1] for m in margins)])
    data["lidar_json"] = np.asarray(json.dumps({"cells": list(CELLS_EXTRA), "maximum_range": 60.0, "normalize": True}))
    return data


# ---- door_crafted: hand-placed roads on a reference MergeEnv --------------------------------------------------------------------------
# cells 16 (cell k looks along k * 22.5 degrees, cell 0 spans +-11.25 degrees), maximum_range 60, raw values.  Slot 0 is the observer
# at (100, 4), heading 0, 25 m/s.  `vehicles`: (x, y, heading, speed) of slots 1.. (the slots a road does not use stand far away);
# `obstacle`: (x, y) of the Obstacle (None: far away); `absent`: (slot, x, y, heading, speed) -- the vehicle of that slot is REMOVED from
# the reference's road and the slot's planes are written as if it stood there.  TIE: equal distances, exact by construction.
OBSERVER = (100.0, 4.0, 0.0, 25.0)
TIE = "tie"
CRAFTED = [
    # 0  TIE: the rear face of a vehicle (132.5 - 2.5) and the near face of the Obstacle (131 - 1) both 30.0 m along the ray of cell 0:
    #    the Obstacle is traced last and wins, -25 m/s instead of -5.  With a vehicle's length its face would stand at 128.5.
    dict(vehicles=[(132.5, 4.5, 0.0, 20.0)], obstacle=(131.0, 3.5), mark=TIE),
    # 1  TIE of the centre candidates of a vehicle and the Obstacle mirrored about the observer's lateral axis, both in cell 4, whose ray
    #    (x = 100) passes between them: equal f64 distances against the float32 the first one stored (the reference's `<=`)
    dict(vehicles=[(103.0, 24.0, 1.0, 10.0)], obstacle=(97.0, 24.0), mark=TIE),
    # 2  an Obstacle straight behind: its corners straddle +-pi
    dict(vehicles=[], obstacle=(80.0, 4.0)),
    # 3  an Obstacle around the boundary between cell 15 and cell 0 (-11.25 degrees): start = 15 >= end = 0
    dict(vehicles=[], obstacle=(120.0, 0.0)),
    # 4  the Obstacle's centre 60.5 m ahead (beyond the range), its near corners at 59.5 m: not traced
    dict(vehicles=[], obstacle=(160.5, 4.0)),
    # 5  ... and the converse: centre at 59.5 m, far corners beyond the range: traced
    dict(vehicles=[], obstacle=(159.5, 4.0)),
    # 6  the observer overlapping the Obstacle: negative centre distance
    dict(vehicles=[(110.0, 8.0, 0.3, 12.0)], obstacle=(100.3, 4.2)),
    # 7  an absent slot placed where it would be hit (15 m ahead), a vehicle behind it that IS hit, the Obstacle to the right
    dict(vehicles=[(130.0, 4.0, 0.0, 20.0)], obstacle=(110.0, -6.0), absent=(2, 115.0, 4.0, 0.0, 10.0)),
    # 8  rotated vehicles and the Obstacle at once, one vehicle with a vehicle's length exactly where the Obstacle's length matters
    dict(vehicles=[(110.0, 0.0, 0.7, 18.0), (95.0, 9.0, -1.2, 15.0), (104.0, 12.0, 2.9, 12.0)], obstacle=(112.0, 9.0)),
]
CRAFTED_SLOTS = 6


def run_crafted() -> dict:
    ref_stub.restore_class_defaults()
    config = {"observation": lidar(cells=16, maximum_range=60, normalize=False)}
    recs, tab0 = [], None
    for road in CRAFTED:
        env = MergeEnv(dict(config))
        env.reset(seed=0)
        vs, objs = env.road.vehicles, env.road.objects
        assert len(vs) == CRAFTED_SLOTS - 1 and len(objs) == 1 and vs[0] is env.vehicle and len(road["vehicles"]) < len(vs)
        placed = [OBSERVER] + list(road["vehicles"])
        placed += [(5000.0 + 100.0 * k, 0.0, 0.0, 20.0) for k in range(len(vs) - len(placed))]
        for v, (x, y, h, s) in zip(vs, placed):
            v.position = np.array([x, y])
            v.heading, v.speed = h, s
        objs[0].position = np.array(road["obstacle"] if road.get("obstacle") else (9000.0, 0.0))
        tab, index = mgm.lane_table(env.road.network)
        tab0 = tab if tab0 is None else tab0
        absent = road.get("absent")
        if absent:
            full = mgm.dump_state(env, index, CRAFTED_SLOTS)
            del vs[absent[0]]
        obs0 = np.asarray(env.observation_type.observe())[None]
        st = mgm.dump_state(env, index, CRAFTED_SLOTS)
        if absent:  # the reference's list is one shorter; the slots keep their places, the removed one is absent and stands in the way
            k = absent[0]
            for key in st:
                st[key] = np.concatenate([st[key][:k], full[key][k:k + 1], st[key][k:CRAFTED_SLOTS - 2], st[key][CRAFTED_SLOTS - 1:]])
            st["present"][k] = 0
            st["x"][k], st["y"][k], st["heading"][k], st["speed"][k] = absent[1:]
        recs.append({"init": st, "obs0": obs0, "cfg": dict(env.config)})
    E = len(recs)
    out = {"seeds": np.zeros(E, np.int64), "actions": np.zeros((0, E, 1), np.int32)}
    out["meta"] = np.asarray([E, CRAFTED_SLOTS, 15, 0, 0, 1], np.int64)
    cfg = recs[0]["cfg"]
    out["cfg_json"] = np.asarray(json.dumps({k: v for k, v in cfg.items() if isinstance(v, (int, float, str, bool, list, dict, type(None)))}))
    out["cfg_generic"] = np.int64(0)
    out["end_position"] = np.float64(370.0)
    for k in mgm.LANE_F64 + mgm.LANE_I32:
        out["lane_" + k] = tab0[k]
    out["obs0"] = np.stack([r["obs0"] for r in recs])  # [E, 1, 16, 2]
    assert out["obs0"].dtype == np.float32
    for k in mgm.F64_FIELDS + mgm.I8_FIELDS:
        out["init_" + k] = np.stack([r["init"][k] for r in recs])
    out["ties"] = np.asarray([int(r.get("mark") == TIE) for r in CRAFTED], np.int8)
    out["lidar_json"] = np.asarray(json.dumps(lidar_of(config)))
    out["margins"] = np.asarray(merge_margins("door_crafted", out, ("init",), 16, 60.0))
    # what each road is for, checked on the reference's own answer
    o = out["obs0"][:, 0]
    assert o[0, 0, 0] == 30.0 and o[0, 0, 1] == -25.0, o[0, 0]       # the Obstacle wins the tie
    assert (o[4] == 60.0).all() and (o[5] != 60.0).any()              # centre beyond the range: skipped; within: traced
    assert o[6].min() < 0                                             # negative centre distance
    assert o[7, 0, 0] == 27.5 and o[7, 0, 1] == -5.0, o[7, 0]         # the absent slot at 115 m is not hit, the vehicle behind it is
    return out


NAMES = [sc["name"] for sc in MERGE + IX] + ["door_cells", "door_crafted"]


def generate(name: str) -> dict:
    for sc in MERGE:
        if sc["name"] == name:
            return run_merge(sc)
    for sc in IX:
        if sc["name"] == name:
            return run_ix(sc)
    return run_cells(CELLS) if name == "door_cells" else run_crafted()


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
        print(f"{name}: meta={data['meta'].tolist()} obs0 {data['obs0'].shape} margins (angle rad, range m)={data['margins'].tolist()} "
              f"-> {os.path.getsize(path) / 1024:.0f} KiB")
    with open(mpath, "w") as fh:
        json.dump(dict(sorted(manifest.items())), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
