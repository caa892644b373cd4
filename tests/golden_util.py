"""Helpers to load the golden fixtures recorded from the unmodified reference
(tests/golden/make_golden.py) into the engine's SoA layout."""
from __future__ import annotations

import json
import os

import numpy as np

from highwayenv_amd import _abi

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tests/golden/MANIFEST.json: for every committed fixture, a digest of its arrays and of the sources that made it, written by the
# generator that wrote the fixture (record_fixture); tests/test_fixture_freshness.py holds the committed files to it
MANIFEST = os.path.join(GOLDEN_DIR, "MANIFEST.json")
SHARED_SOURCES = ["oracle/ref_stub.py"]   # (every generator imports the reference through it)


def arrays_digest(data) -> str:
    """sha256 over the arrays of a fixture (name, dtype, shape and bytes of each, in name order): what np.load gives back, not the
    .npz container (whose zip entries carry timestamps)."""
    import hashlib
    h = hashlib.sha256()
    for k in sorted(data.files if hasattr(data, "files") else data):
        a = np.ascontiguousarray(np.asarray(data[k]))
        h.update(f"{k}|{a.dtype.str}|{a.shape}|".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def json_fixture_arrays(obj) -> dict:
    """A JSON fixture as the one array its manifest entry digests."""
    return {"json": np.asarray(json.dumps(obj, sort_keys=True))}


def sources_digest(sources) -> str:
    """sha256 over source files (paths relative to the repository root, in the order given)."""
    import hashlib
    h = hashlib.sha256()
    for rel in sources:
        h.update(rel.encode() + b"|")
        with open(os.path.join(ROOT, rel), "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def load_manifest() -> dict:
    with open(MANIFEST) as f:
        return json.load(f)


def fixture_arrays(path: str):
    """The arrays of the committed fixture `path` (relative to tests/golden) as its manifest entry digests them."""
    full = os.path.join(GOLDEN_DIR, path)
    if full.endswith(".json"):
        with open(full) as f:
            return json_fixture_arrays(json.load(f))
    return np.load(full)


def record_fixture(name: str, path: str, sources) -> None:
    """Called by a generator right after it wrote fixture `name` (`path`, relative to tests/golden) from `sources`."""
    sources = list(sources) + SHARED_SOURCES
    manifest = load_manifest() if os.path.exists(MANIFEST) else {}
    manifest[name] = {"path": path, "arrays_sha256": arrays_digest(fixture_arrays(path)), "sources": sources,
                      "sources_sha256": sources_digest(sources)}
    with open(MANIFEST, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")

GRID = ["grid_default", "grid_aligned_fine", "grid_xy_range", "grid_image"]
ALL = ["cfg1_fast_default", "cfg2_fast_n50_l4", "v0_default", "cfg3_v0_n100", "dense_crash",
       "fast_idle_long", "fast_offroad_terminal", "fast_lateral_only", "v0_longitudinal_only"]
WITH_FRAMES = ["cfg1_fast_default", "cfg2_fast_n50_l4", "v0_default", "cfg3_v0_n100", "dense_crash",
               "fast_lateral_only", "v0_longitudinal_only"]


class _InMemory:
    """What np.load gives for a committed fixture, for a trace held in memory (tests/test_oracle_live_reference.py:
    a recorded trace of tests/golden/live, or the generators' run_scenario output of a live run)."""

    def __init__(self, data: dict):
        self._d = {k: np.asarray(v) for k, v in data.items()}
        self.files = list(self._d)

    def __getitem__(self, k):
        return self._d[k]

    def __contains__(self, k):
        return k in self._d


def _load(name: str, data):
    return _InMemory(data) if data is not None else np.load(os.path.join(GOLDEN_DIR, name + ".npz"))


class Golden:
    def __init__(self, name: str, data: dict | None = None):
        self.name = name
        self.z = _load(name, data)
        z = self.z
        self.E, self.N, self.T, self.steps, self.frames_for = (int(v) for v in z["meta"])
        self.fast = bool(z["cfg_fast"])
        self.config = (_abi.highway_fast_default_config() if self.fast else _abi.highway_default_config())
        self.config.update({
            "lanes_count": int(z["cfg_lanes_count"]),
            "vehicles_count": int(z["cfg_vehicles_count"]),
            "simulation_frequency": int(z["cfg_simulation_frequency"]),
            "policy_frequency": int(z["cfg_policy_frequency"]),
            "duration": float(z["cfg_duration"]),
            "ego_spacing": float(z["cfg_ego_spacing"]),
            "vehicles_density": float(z["cfg_vehicles_density"]),
            "normalize_reward": bool(z["cfg_normalize_reward"]),
            "offroad_terminal": bool(z["cfg_offroad_terminal"]),
            "collision_reward": float(z["cfg_collision_reward"]),
            "right_lane_reward": float(z["cfg_right_lane_reward"]),
            "high_speed_reward": float(z["cfg_high_speed_reward"]),
            "reward_speed_range": [float(v) for v in z["cfg_reward_speed_range"]],
        })
        if "cfg_observation_json" in z.files:
            import json
            self.config["observation"] = json.loads(str(z["cfg_observation_json"]))
        if "cfg_action_json" in z.files:
            import json
            self.config["action"] = json.loads(str(z["cfg_action_json"]))
        self.seeds = z["seeds"]
        self.actions = z["actions"]  # [steps, E]

    def hwy_config(self, num_envs=None) -> _abi.HwyConfig:
        return _abi.make_config(self.config, self.E if num_envs is None else num_envs)

    def state(self, prefix: str, index=None, envs=None, time=0.0) -> dict:
        """SoA dict from `init_*` (index None), `step_*[index]` or `frame_*[index]`."""
        z = self.z

        def get(k):
            a = z[f"{prefix}_{k}"]
            if index is not None:
                a = a[index]
            if envs is not None:
                a = a[envs]
            return a

        E = get("x").shape[0]
        st = _abi.alloc_state(E, self.N)
        for k in ["x", "y", "heading", "speed", "target_speed", "impact_x", "impact_y"]:
            st[k][...] = get(k)
        st["timer"][...] = np.nan_to_num(get("timer"), nan=0.0)
        st["delta"][...] = np.nan_to_num(get("delta"), nan=0.0)
        st["lane"][...] = get("lane")
        st["target_lane"][...] = get("target_lane")
        st["speed_index"][...] = np.maximum(get("speed_index"), 0)
        st["flags"][...] = (get("crashed") * _abi.F_CRASHED + get("has_impact") * _abi.F_HAS_IMPACT
                            + get("check_collisions") * _abi.F_CHECK_COLLISIONS
                            + get("controlled") * _abi.F_CONTROLLED)
        st["time"][...] = time
        return st


# HWY_STRICT_TOL=1 -- a knob that only tightens (tests/test_strict_arithmetic.py sets it in the child processes that run an unfused
# build): the lateral offset of slow intersection cars goes back from the 1e-6 the fused build needs to the 1e-8 the unfused build
# of rounds 1-3 held (highwayenv_amd/build.py FP_CONTRACT).  Rounds 1-3 had no bound of their own for slow
# cars: they were held to the comparison's `atol`, so on the step of a collision (atol 1e-6) the slow bound is that atol.
STRICT_TOL = os.environ.get("HWY_STRICT_TOL") == "1"
STRICT_SLOW_ATOL = 1e-8


def slow_tolerance(slow_atol, atol):
    """The tolerance for slow intersection cars: the caller's, or -- HWY_STRICT_TOL=1 -- the unfused build's if that is tighter."""
    if slow_atol is None or not STRICT_TOL:
        return slow_atol
    return min(slow_atol, max(STRICT_SLOW_ATOL, atol))


KNIFE = 1e-9  # |d.normal| below which the SIGN of a collision push is decided by the last bit of the libm in use


def _assert_impacts(got, want, rows, atol, what, signed=None):
    """Pending impacts on `rows` [E, N]: SIGNED where `signed` [E, N] says the collision is well conditioned (oracle.impact_margins
    >= KNIFE), otherwise up to a global sign.  The reference orients the minimum-translation vector with `d.dot(normal) > 0`
    (utils.py:232-236); for two cars tracking the same lane centre d.normal is rounding noise (~1e-16) and its sign differs
    between any two libm implementations."""
    for k in ["impact_x", "impact_y"]:
        np.testing.assert_allclose(np.abs(got[k][rows]), np.abs(want[k][rows]), rtol=0, atol=atol, err_msg=f"{what}: |{k}|")
        if signed is not None:
            m = rows & signed
            np.testing.assert_allclose(got[k][m], want[k][m], rtol=0, atol=atol, err_msg=f"{what}: signed {k}")


def mask_knife_edge_flags(got: dict, want: dict, flag_margin) -> None:
    """A wreck pushed back by its impact rests EXACTLY touching what it hit; from then on `intersecting` (utils.py:222-224: the
    partner's crashed flag -- in practice the never-pushed Obstacle's) hinges on a distance of ~0 (oracle.impact_margins.flag_margin
    < KNIFE).  On those slots the crashed / has-impact BITS of `got` are taken from `want`, and so is the PENDING IMPACT: a pair
    found touching overwrites the slot's impact with its own ~0 translation (the last colliding pair wins, objects.py:104-112), a
    pair found apart leaves the impact of an earlier, real collision in place -- either is the reference's answer for one of the
    two roundings.  Positions and speeds stay compared (a flipped decision moves nothing by more than the ~0 distance it hinges
    on before the impact is applied; the callers re-synchronise wrecked environments)."""
    edge = np.asarray(flag_margin) < KNIFE
    bits = _abi.F_CRASHED | _abi.F_HAS_IMPACT
    got["flags"][edge] = (got["flags"][edge] & ~bits) | (want["flags"][edge] & bits)
    for k in ["impact_x", "impact_y"]:
        got[k][edge] = want[k][edge]


def assert_state_close(got: dict, want: dict, atol=1e-9, what=""):
    for k in ["lane", "target_lane", "flags"]:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")
    ctrl = (want["flags"] & _abi.F_CONTROLLED) != 0
    np.testing.assert_array_equal(got["speed_index"][ctrl], want["speed_index"][ctrl], err_msg=f"{what}: speed_index")
    for k in ["x", "y", "heading", "speed", "target_speed"]:
        np.testing.assert_allclose(got[k], want[k], rtol=0, atol=atol, err_msg=f"{what}: {k}")
    # pending impacts: compared up to a global sign.  The reference orients the minimum-translation
    # vector with `d.dot(normal) > 0` (utils.py:232-236); for two cars tracking the same lane centre
    # d.normal is rounding noise (~1e-16) and its sign differs between any two libm implementations.
    for k in ["impact_x", "impact_y"]:
        np.testing.assert_allclose(np.abs(got[k]), np.abs(want[k]), rtol=0, atol=atol, err_msg=f"{what}: |{k}|")
    np.testing.assert_allclose(got["timer"][~ctrl], want["timer"][~ctrl], rtol=0, atol=atol, err_msg=f"{what}: timer")


IMAGE_CELLS = [0, 0]  # as_image cells that differed by one uint8 step / cells compared, engine vs oracle, this session


def assert_obs_close(got, want, image: bool, what="", atol=1e-6):
    """Observations of the engine vs the oracle on the SAME state: 1e-6 (callers pass 2.5e-6 for the step of a collision, whose
    positions are compared at 1e-6: an un-normalised relative feature is the difference of two of them), or --
    OccupancyGrid(as_image=True) -- equal up to one uint8 step in a handful of cells: uint8(((v + 1) / 2) * 255) jumps where the
    product is an integer (cos_h = 1 - 1e-17 -> 254 or 255), and two libms land on either side of such a jump."""
    if not image:
        np.testing.assert_allclose(got, want, rtol=0, atol=atol, err_msg=what)
        return
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    IMAGE_CELLS[0] += int((d > 0).sum())   # reported in the terminal summary (tests/conftest.py)
    IMAGE_CELLS[1] += int(d.size)
    assert d.max(initial=0) <= 1.0 and (d > 0).sum() <= max(2, 1e-3 * d.size), f"{what}: {int((d > 0).sum())} cells differ, max {d.max(initial=0)}"


# --------------------------------------------------------------------------- merge scenarios
MERGE = ["merge_default", "merge_generic_l3", "merge_generic_sections", "merge_ma4", "merge_v1", "merge_generic_v1",
         "merge_no_obstacles"]
MERGE_GRID = ["merge_grid", "merge_generic_grid_aligned", "merge_grid_image"]  # per-step fixtures with the OccupancyGrid observation
# crash-rich (round 3): dense merge-generic traffic, the 4-agent config-5 shape, vehicle-vs-Obstacle hits (an ego placed on the
# acceleration lane: its reset is the generator's, not MergeEnv's)
MERGE_CRASH = ["merge_crash_generic", "merge_crash_ma4", "merge_crash_obstacle"]


class GoldenMerge:
    """Fixtures of tests/golden/make_golden_merge.py (MergeEnv / MergeGenericEnv)."""

    def __init__(self, name: str, data: dict | None = None):
        import json

        from highwayenv_amd import merge
        self.name = name
        self.z = z = _load(name, data)
        self.E, self.N, self.T, self.steps, self.frames_for, self.A = (int(v) for v in z["meta"])
        self.generic = bool(z["cfg_generic"])
        self.scenario = "merge-generic" if self.generic else "merge"
        self.config = merge.merge_generic_default_config() if self.generic else merge.merge_default_config()
        self.config.update(json.loads(str(z["cfg_json"])))
        self.seeds = z["seeds"]
        self.actions = z["actions"]  # [steps, E, A]

    def hwy_config(self, num_envs=None) -> _abi.HwyConfig:
        return _abi.make_config(self.config, self.E if num_envs is None else num_envs, scenario=self.scenario)

    def state(self, prefix: str, index=None, envs=None, time=0.0) -> dict:
        z = self.z

        def get(k):
            a = z[f"{prefix}_{k}"]
            if index is not None:
                a = a[index]
            if envs is not None:
                a = a[envs]
            return a

        E = get("x").shape[0]
        st = _abi.alloc_state(E, self.N)
        for k in ["x", "y", "heading", "speed", "target_speed", "impact_x", "impact_y", "timer", "delta"]:
            st[k][...] = get(k)
        for k in ["lane", "target_lane", "speed_index"]:
            st[k][...] = get(k)
        st["flags"][...] = (get("crashed") * _abi.F_CRASHED + get("has_impact") * _abi.F_HAS_IMPACT
                            + get("check_collisions") * _abi.F_CHECK_COLLISIONS
                            + get("controlled") * _abi.F_CONTROLLED + get("obstacle") * _abi.F_OBSTACLE
                            + (1 - get("present")) * _abi.F_ABSENT)
        st["time"][...] = time
        return st


def assert_net_state_close(got: dict, want: dict, atol=1e-9, what="", signed=None):
    """assert_state_close for the road-network scenarios (absent slots ignored); `signed` [E, N]: see _assert_impacts."""
    pres = (want["flags"] & _abi.F_ABSENT) == 0
    np.testing.assert_array_equal((got["flags"] & _abi.F_ABSENT) == 0, pres, err_msg=f"{what}: present")
    for k in ["lane", "target_lane", "flags"]:
        np.testing.assert_array_equal(got[k][pres], want[k][pres], err_msg=f"{what}: {k}")
    ctrl = pres & ((want["flags"] & _abi.F_CONTROLLED) != 0)
    idm = pres & ((want["flags"] & (_abi.F_CONTROLLED | _abi.F_OBSTACLE)) == 0)
    np.testing.assert_array_equal(got["speed_index"][ctrl], want["speed_index"][ctrl], err_msg=f"{what}: speed_index")
    for k in ["x", "y", "heading", "speed", "target_speed"]:
        np.testing.assert_allclose(got[k][pres], want[k][pres], rtol=0, atol=atol, err_msg=f"{what}: {k}")
    _assert_impacts(got, want, pres, atol, what, signed)
    np.testing.assert_allclose(got["timer"][idm], want["timer"][idm], rtol=0, atol=atol, err_msg=f"{what}: timer")


INTERSECTION = ["intersection_default", "intersection_dense", "intersection_v2"]   # per-frame fixtures (Kinematics observation)
INTERSECTION_CRASH = ["intersection_crash", "intersection_crash_ma3"]  # crash-rich (round 3), per-frame states for the first envs
INTERSECTION_GRID = ["intersection_grid", "intersection_grid_aligned", "intersection_grid_image"]  # per-step fixtures, OccupancyGrid observation
# MultiAgentIntersectionEnv (2 agents with per-frame states; 3 agents with random destinations, per-step states only)
INTERSECTION_MA = ["intersection_multi_agent", "intersection_multi_agent3"]
INTERSECTION_MA_FRAMES = ["intersection_multi_agent"]
# the destination features cos_d / sin_d with and without observe_intentions, the lane-offset features (per-step fixtures)
INTERSECTION_INTENTIONS = ["intersection_intentions", "intersection_no_intentions", "intersection_lane_offsets"]


class GoldenIntersection:
    """Fixtures of tests/golden/make_golden_intersection.py (IntersectionEnv); state dicts for oracle/oracle_ix.py."""

    def __init__(self, name: str, data: dict | None = None):
        import json

        from oracle import oracle_ix
        self.ix = oracle_ix
        self.name = name
        self.z = z = _load(name, data)
        self.E, self.N, self.T, self.steps, self.frames_for, self.A, self.R = (int(v) for v in z["meta"])
        self.config = json.loads(str(z["cfg_json"]))
        self.actions = z["actions"]  # [steps, E, A]
        self.lane_tab = {k: z["lane_" + k] for k in oracle_ix.LANE_F64 + oracle_ix.LANE_I32}

    def ix_config(self, num_envs=None):
        return self.ix.make_config(self.config, self.lane_tab, self.z["node_names"],
                                   self.E if num_envs is None else num_envs, self.N, self.R)

    def state(self, prefix: str, index=None, envs=None, road_steps=None, time=0.0) -> dict:
        z = self.z

        def get(k):
            a = z[f"{prefix}_{k}"]
            if index is not None:
                a = a[index]
            if envs is not None:
                a = a[envs]
            return a

        E = get("x").shape[0]
        st = self.ix.alloc_state(E, self.N, self.R)
        for k in self.ix.STATE_F64 + self.ix.STATE_I32 + self.ix.STATE_ROUTE:
            st[k][...] = get(k)
        st["vid"] = np.array(get("vid"))
        if road_steps is not None:
            st["road_steps"][...] = road_steps
        st["time"][...] = time
        return st


def assert_ix_state_close(got: dict, want: dict, atol=1e-9, what="", signed=None, slow_atol=None, slow_start=None, slow_below=2.0):
    """`slow_atol`: the tolerance for vehicles below `slow_below` m/s at either end of the compared interval (`slow_start`: their
    speeds at its start) -- see assert_ix_engine_state_close."""
    pres = want["present"] != 0
    np.testing.assert_array_equal(got["present"] != 0, pres, err_msg=f"{what}: present")
    for k in ["lane", "target_lane", "crashed", "has_impact", "controlled", "is_yielding", "route_len"]:
        np.testing.assert_array_equal(got[k][pres], want[k][pres], err_msg=f"{what}: {k}")
    for k in ["route_from", "route_to", "route_id"]:
        m = pres[..., None] & (np.arange(want[k].shape[-1]) < want["route_len"][..., None])
        np.testing.assert_array_equal(got[k][m], want[k][m], err_msg=f"{what}: {k}")
    ctrl = pres & (want["controlled"] != 0)
    np.testing.assert_array_equal(got["speed_index"][ctrl], want["speed_index"][ctrl], err_msg=f"{what}: speed_index")
    slow_atol = slow_tolerance(slow_atol, atol)
    slow = np.zeros_like(pres)
    if slow_atol is not None:
        slow = pres & ((np.abs(want["speed"]) < slow_below) | (np.abs(got["speed"]) < slow_below))
        if slow_start is not None:
            slow |= pres & (np.abs(slow_start) < slow_below)
    for k in ["x", "y", "heading", "speed", "target_speed"]:
        np.testing.assert_allclose(got[k][pres & ~slow], want[k][pres & ~slow], rtol=0, atol=atol, err_msg=f"{what}: {k}")
        if slow.any():
            np.testing.assert_allclose(got[k][slow], want[k][slow], rtol=0, atol=slow_atol, err_msg=f"{what}: {k} (below {slow_below} m/s)")
    _assert_impacts(got, want, pres, atol, what, signed)
    idm = pres & (want["controlled"] == 0)
    np.testing.assert_allclose(got["timer"][idm], want["timer"][idm], rtol=0, atol=atol, err_msg=f"{what}: timer")


def ix_engine_state(g: "GoldenIntersection", gst: dict, cfg) -> dict:
    """Golden / oracle intersection state (tests' own layout) -> the product's hwy_state dict for hwy_set_state."""
    from highwayenv_amd import intersection as hix
    tab = hix.table_from_config(cfg)
    E = gst["x"].shape[0]
    st = _abi.alloc_state_ix(E, cfg.num_vehicles)
    n = g.N
    assert n <= cfg.num_vehicles
    for k in ["x", "y", "heading", "speed", "timer", "target_speed", "delta", "impact_x", "impact_y"]:
        st[k][:, :n] = gst[k]
    for k in ["lane", "target_lane", "speed_index"]:
        st[k][:, :n] = gst[k]
    pres = gst["present"] != 0
    flags = (gst["crashed"] * _abi.F_CRASHED + gst["has_impact"] * _abi.F_HAS_IMPACT + _abi.F_CHECK_COLLISIONS
             + gst["controlled"] * _abi.F_CONTROLLED + gst["is_yielding"] * _abi.F_YIELDING)
    st["flags"][:, :n] = np.where(pres, flags, _abi.F_ABSENT)
    lane_of = {(int(tab["from_node"][k]), int(tab["to_node"][k])): k for k in range(len(tab["kind"]))}
    for e in range(E):
        for i in np.nonzero(pres[e])[0]:
            r = [lane_of[(int(gst["route_from"][e, i, q]), int(gst["route_to"][e, i, q]))] for q in range(int(gst["route_len"][e, i]))]
            st["route"][e, i] = hix.route_pack(r)
    st["road_steps"][...] = gst["road_steps"]
    st["time"][...] = gst["time"]
    return st


def assert_ix_engine_state_close(got: dict, want: dict, atol=1e-9, what="", signed=None, slow_atol=None, slow_below=2.0,
                                 slow_start=None):
    """Two hwy_state dicts of the intersection scenario (absent slots ignored).  `slow_atol`: the tolerance for vehicles
    below `slow_below` m/s at either end of the compared interval (`slow_start` = their speeds at its start): steering_control
    divides by not_zero(speed) twice, so a last-bit difference of two arithmetics (libm, fused multiply-add or not) grows
    1e2 x faster per frame on a car that yields or queues than on one that drives."""
    pres = (want["flags"] & _abi.F_ABSENT) == 0
    np.testing.assert_array_equal((got["flags"] & _abi.F_ABSENT) == 0, pres, err_msg=f"{what}: present")
    for k in ["lane", "target_lane", "flags", "route"]:
        np.testing.assert_array_equal(got[k][pres], want[k][pres], err_msg=f"{what}: {k}")
    ctrl = pres & ((want["flags"] & _abi.F_CONTROLLED) != 0)
    np.testing.assert_array_equal(got["speed_index"][ctrl], want["speed_index"][ctrl], err_msg=f"{what}: speed_index")
    slow_atol = slow_tolerance(slow_atol, atol)
    slow = np.zeros_like(pres)
    if slow_atol is not None:
        slow = pres & ((want["speed"] < slow_below) | (got["speed"] < slow_below))
        if slow_start is not None:
            slow |= pres & (slow_start < slow_below)
    for k in ["x", "y", "heading", "speed", "target_speed"]:
        np.testing.assert_allclose(got[k][pres & ~slow], want[k][pres & ~slow], rtol=0, atol=atol, err_msg=f"{what}: {k}")
        if slow.any():
            np.testing.assert_allclose(got[k][slow], want[k][slow], rtol=0, atol=slow_atol, err_msg=f"{what}: {k} (below {slow_below} m/s)")
    _assert_impacts(got, want, pres, atol, what, signed)
    idm = pres & ~ctrl
    np.testing.assert_allclose(got["timer"][idm], want["timer"][idm], rtol=0, atol=atol, err_msg=f"{what}: timer")
    np.testing.assert_array_equal(got["road_steps"], want["road_steps"], err_msg=f"{what}: road_steps")


def ix_oracle_state(h: dict, cfg) -> dict:
    from oracle import oracle_ix
    return oracle_ix.state_from_engine(h, cfg)


def ix_oracle_config(cfg_dict: dict, cfg, num_envs: int):
    from oracle import oracle_ix
    return oracle_ix.config_from_engine(cfg_dict, cfg, num_envs)


class OraclePool:
    """The C oracle over ALL environments of a full-size batch: disjoint blocks of environments, one block per thread of a pool
    (ctypes releases the GIL inside the C call; the oracle's diagnostic buffers are thread-local), so that the full-size parity
    tests compare every environment of BASELINE configs 3 / 4 / 5 instead of a sample -- like bench.py's cpu_baseline leg steps the
    same oracle on every host core.  ``make_cfg(n)`` builds the oracle's config for a block of n environments."""

    def __init__(self, num_envs: int, make_cfg, threads: int | None = None):
        import os
        from concurrent.futures import ThreadPoolExecutor
        n = max(1, min(threads or (os.cpu_count() or 1), 64, num_envs))
        edges = np.linspace(0, num_envs, n + 1).astype(int)
        self.blocks = [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:]) if b > a]
        self.cfgs = [make_cfg(b - a) for a, b in self.blocks]
        self.pool = ThreadPoolExecutor(len(self.blocks))
        self.num_envs = num_envs

    def split(self, arrays: dict) -> list:
        """[E, ...] arrays -> one contiguous copy per block (the oracle steps its block in place)."""
        return [{k: np.ascontiguousarray(v[a:b]).copy() for k, v in arrays.items()} for a, b in self.blocks]

    def run(self, fn, *per_block):
        """fn(cfg_k, margins_k, *[x[k] for x in per_block]) on every block in parallel; the list of results in block order."""
        from oracle import oracle

        def one(k):
            with oracle.impact_margins(self.cfgs[k]) as mg:
                return fn(self.cfgs[k], mg, *[x[k] for x in per_block]), mg.margin.min(1), mg.flag_margin.min(1)
        return list(self.pool.map(one, range(len(self.blocks))))

    def rows(self, x):
        return [x[a:b] for a, b in self.blocks]

    def close(self):
        self.pool.shutdown()
