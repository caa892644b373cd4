"""The register-allocation builds of the step and rollout kernels: which configurations reach them, what the engine launches for
each, and the comparison that holds one build to another bit for bit.

A step, rollout or workgroup kernel is compiled once per ``WPE`` -- ``__launch_bounds__(threads, WPE)``, the waves per SIMD the
register allocator leaves room for -- and ``hwy_create`` picks one at run time (``hwy_config.tune_waves_per_eu``, or its own rule on
the batch size).  ``rows()`` has one row per branch of the selection layer (csrc/hwy_launch_family.h, hwy_launch_rules.h) in which
that value picks a build; ``launched()`` restates the selection in Python, FOR THE TESTS ONLY, in the key format of
``highwayenv_amd.build.kernel_resources()``; tests/test_kernel_variants.py holds the two to the code object's own list of kernels
(both ways) and runs every (row, value) on the MI355X against the build the engine takes by default.  tools/launch_table.py imports
the rows, so there is one list."""
from __future__ import annotations

import re

import numpy as np

from highwayenv_amd import _abi

LINEAR = "highway_env.vehicle.behavior.LinearVehicle"
AGGRESSIVE = "highway_env.vehicle.behavior.AggressiveVehicle"
GRID = {"observation": {"type": "OccupancyGrid"}}
DIRECT = {"action": {"type": "DiscreteAction", "steering_range": [-0.1, 0.1]}}
BLOCK = {"tuning": {"block_kernel": 1}}
# the step and rollout kernels among the keys of kernel_resources(): hwy_[net_|ix_](step|rollout)[_wave|_wide][_linear|_direct]_kernel<...>
STEP_OR_ROLLOUT = re.compile(r"^hwy::hwy_(?:[a-z]+_)?(?:step|rollout)_(?:[a-z_]+_)?kernel<")
# the one-wavefront step kernel compiled for a registered configuration (csrc/hwy_wave.h: FixedShape; hwy_kernels_shapes.hip)
SHAPE_KERNEL = re.compile(r"^hwy::hwy_shape_wave_kernel<")
# shape id (hwy_last_step_shape) -> (lanes, hwy_config.flags, frames per policy step) of FastShape3, FastShape4 and V0Shape4
_V0_FLAGS = _abi.C_OBS_NORMALIZE | _abi.C_OBS_CLIP | _abi.C_NORMALIZE_REWARD
SHAPES = {1: (3, _V0_FLAGS | _abi.C_EGO_ONLY_COLLISIONS, 5), 2: (4, _V0_FLAGS | _abi.C_EGO_ONLY_COLLISIONS, 5), 3: (4, _V0_FLAGS, 15)}
SHAPE_NAMES = {1: "FastShape3", 2: "FastShape4", 3: "V0Shape4"}  # (csrc/hwy_wave.h)


def label_shape(label: str) -> int:
    """The shape id a row's label names (0: none): a row says in its label which kernel its step() runs."""
    named = [shape for shape, name in SHAPE_NAMES.items() if name in label]
    assert len(named) <= 1, label
    return named[0] if named else 0


def hwy(n: int, **over) -> dict:
    """highway-v0 with n vehicles in all: episodes of 3 policy steps, so that every environment ends and is re-spawned within a
    short run, and twice the default density, so that lane changes and collisions happen in it."""
    d = _abi.highway_default_config()
    d.update({"vehicles_count": n - 1, "duration": 3, "vehicles_density": 2.0, **over})
    return d


def fast(n: int, lanes: int, **over) -> dict:
    """highway-fast-v0's structure (5 frames per policy step; with make_config's fast=True: ego-only collisions) with n vehicles in
    all on `lanes` lanes: episodes of 3 policy steps and twice the default density, like hwy()."""
    d = _abi.highway_fast_default_config()
    d.update({"vehicles_count": n - 1, "lanes_count": lanes, "duration": 3, "vehicles_density": 2.0, **over})
    return d


def merge_row() -> dict:
    """merge-generic: 3 lanes, 20 vehicles, 2 agents.  A road-network episode is never truncated: it ends with a crash or when the
    ego passes `road length - 90 m`.  The sections are cut to 30 m each, so that the ego (spawned at x = 30 m with 30 m/s) is past
    the end (90 m) after two or three policy steps and every environment is re-spawned within four."""
    from highwayenv_amd import merge
    d = merge.merge_generic_default_config()
    d.update({"lanes_count": 3, "vehicles_count": 20, "controlled_vehicles": 2,
              "before_merge_length": 30, "converge_merge_length": 30, "parallel_merge_length": 30, "after_merge_length": 90,
              "action": {"type": "MultiAgentAction", "action_config": {"type": "DiscreteMetaAction"}},
              "observation": {"type": "MultiAgentObservation", "observation_config": {"type": "Kinematics"}}})
    return d


def ix(slots: int, **over) -> dict:
    from highwayenv_amd import intersection
    d = intersection.intersection_default_config()
    d.update({"max_vehicles": slots, "host_traffic": False, "duration": 3, **over})
    return d


def rows() -> list:
    """(label, config dict, make_config keywords): every branch of the selection in which waves_per_eu picks a build.  N = 64 on the
    one-wavefront kernels: no lane is idle; N = 65 / 129 / 256: two wavefronts of which the second holds ONE vehicle, three, and
    four full ones.  Not here, because the knob selects nothing there and a row would only pass for coverage: the wide kernel
    (hwy_wave2.h: one build per vehicles-per-thread), OccupancyGrid on the road network (<3, true>), the intersection with more
    than 32 slots (<2, 64>), every reset and observe kernel (one build each) and the Lidar kernel."""
    out = [
        # IDM traffic, meta-actions.  The workgroup kernel is forced (block_kernel=1) where the engine would take the one-wavefront
        # or the wide kernel; the OccupancyGrid row is the engine's own route to it for N > 64.
        # The registered configurations run the kernel compiled for them on every step() (auto-reset is on in every comparison:
        # step_shape); their rollout() and the rows beside them run the generic one-wavefront kernel: highway-v0's structure
        # with ego-only collisions (15 frames per step: no shape) and highway-v0 on 5 lanes (no shape has 5)
        ("idm wave ego-only N=64", hwy(64), {"fast": True}),
        ("idm wave full-scan N=64 generic L=5", hwy(64, lanes_count=5), {}),
        ("idm wave full-scan N=64 V0Shape4", hwy(64), {}),
        ("idm wave FastShape3 N=64", fast(64, 3), {"fast": True}),
        ("idm wave FastShape4 N=64", fast(64, 4), {"fast": True}),
        ("idm block NW=1 N=64", hwy(64), dict(BLOCK)),
        ("idm block NW=2 N=65", hwy(65), dict(BLOCK)),
        ("idm block NW=3 N=129", hwy(129), dict(BLOCK)),
        ("idm block NW=4 N=256", hwy(256), dict(BLOCK)),
        ("idm block NW=2 N=65 OccupancyGrid", hwy(65, **GRID), {}),
        # Linear traffic: no wide kernel, the workgroup kernel is the engine's choice above 64
        ("linear wave ego-only N=64", hwy(64, other_vehicles_type=LINEAR), {"fast": True}),
        ("linear wave full-scan N=64", hwy(64, other_vehicles_type=LINEAR), {}),
        ("linear block NW=1 N=64", hwy(64, other_vehicles_type=LINEAR), dict(BLOCK)),
        ("linear block NW=2 N=65", hwy(65, other_vehicles_type=LINEAR), {}),
        ("aggressive block NW=3 N=129", hwy(129, other_vehicles_type=AGGRESSIVE), {}),
        ("linear block NW=4 N=256", hwy(256, other_vehicles_type=LINEAR), {}),
        # direct ego control (DiscreteAction): likewise
        ("direct wave ego-only N=64", hwy(64, **DIRECT), {"fast": True}),
        ("direct wave full-scan N=64", hwy(64, **DIRECT), {}),
        ("direct block NW=1 N=64", hwy(64, **DIRECT), dict(BLOCK)),
        ("direct block NW=2 N=65", hwy(65, **DIRECT), {}),
        ("direct block NW=3 N=129", hwy(129, **DIRECT), {}),
        ("direct block NW=4 N=256", hwy(256, **DIRECT), {}),
        ("merge-generic Kinematics", merge_row(), {"scenario": "merge-generic"}),
        ("intersection N=30 helpers", ix(30), {"scenario": "intersection"}),
        ("intersection N=30 no helpers", ix(30), {"scenario": "intersection", "tuning": {"ix_no_helpers": 1}}),
    ]
    assert len({r[0] for r in out}) == len(out)
    return out


def values(kw: dict) -> tuple:
    """The waves_per_eu values a row is run at: the intersection's rule distinguishes two (1 and 2 -> 2, 3 and 4 -> 3)."""
    return (2, 3) if kw.get("scenario") == "intersection" else (1, 2, 3, 4)


def with_tuning(kw: dict, **knobs) -> dict:
    """make_config keywords with `knobs` added to their tuning."""
    return {**kw, "tuning": {**kw.get("tuning", {}), **knobs}}


def step_shape(d: dict, kw: dict) -> int:
    """The shape id (hwy_last_step_shape: 1 = FastShape3, 2 = FastShape4, 3 = V0Shape4) of the kernel a FULL policy step with
    auto-reset on and every output plane bound launches for a configuration, or 0: the generic kernel.  HWY_FIXED_SHAPE_FIELDS
    (csrc/hwy_wave.h) and step_shape_of (hwy_launch_family.h) restated on the hwy_config: IDM traffic with meta-actions on the
    straight road, at most 64 vehicles, the one-wavefront kernel not overridden, one agent at index 0, the default Kinematics
    observation, three target speeds, the full meta-action table -- and the shape's lanes, flags and frames per step."""
    return step_shape_of_config(_abi.make_config(d, 1, **kw))


def step_shape_of_config(c) -> int:
    if c.scenario != _abi.SCENARIO_HIGHWAY or c.traffic_model != _abi.TRAFFIC_IDM or c.ego_control != _abi.EGO_META:
        return 0
    if c.num_vehicles > 64 or c.tune_block_kernel == 1:
        return 0
    std5 = c.obs_type == _abi.OBS_KINEMATICS and c.obs_features == 5 and list(c.obs_feature_ids[:5]) == [0, 1, 2, 3, 4]
    if not (c.num_agents == 1 and c.agent_index[0] == 0 and std5 and c.obs_vehicles == 5 and c.num_target_speeds == 3
            and c.action_set == _abi.ACTIONS_SET_ALL):
        return 0
    for shape, fixed in SHAPES.items():
        if (c.lanes_count, c.flags, c.frames_per_step) == fixed:
            return shape
    return 0


def shape_kernel(shape: int, waves_per_eu: int) -> str:
    lanes, flags, frames = SHAPES[shape]
    return f"hwy::hwy_shape_wave_kernel<hwy::FixedShape<{shape}, {lanes}, {flags}, {frames}>, {waves_per_eu}>"


def launched(d: dict, kw: dict, waves_per_eu: int) -> tuple:
    """(step kernel, rollout kernel) the engine launches for a configuration whose waves-per-EU value is `waves_per_eu` (1 .. 4:
    hwy_config.tune_waves_per_eu, or what hwy_create chose), as keys of kernel_resources().  The step kernel is that of a full
    step() with auto-reset on, as every comparison here runs it: the kernel compiled for the configuration where it is a
    registered one (step_shape); the rollout kernel is always the generic one.  The selection rules of csrc/hwy_params.h
    (force_block_kernel), hwy_launch_family.h and hwy_launch_rules.h, restated."""
    assert 1 <= waves_per_eu <= 4
    shape = step_shape(d, kw)
    if shape:
        return shape_kernel(shape, waves_per_eu), generic_launched(d, kw, waves_per_eu)[1]
    return generic_launched(d, kw, waves_per_eu)


def generic_launched(d: dict, kw: dict, waves_per_eu: int) -> tuple:
    """launched() with the shape kernels set aside (hwy_step_shapes(0), an engine before hwy_set_autoreset, a frames-only call)."""
    c = _abi.make_config(d, 1, **kw)
    n, w = c.num_vehicles, waves_per_eu
    grid = c.obs_type != _abi.OBS_KINEMATICS
    if c.scenario == _abi.SCENARIO_INTERSECTION:
        if n > 32:
            stem, args = "hwy_ix_{}_kernel", "2, 64, 64"
        else:
            helpers = not c.tune_ix_no_helpers
            stem, args = "hwy_ix_{}_kernel", f"{3 if w >= 3 else 2}, 32, {64 if helpers else 32}"
    elif c.scenario != _abi.SCENARIO_HIGHWAY:
        stem, args = "hwy_net_{}_kernel", "3, true" if grid else f"{w}, false"
    else:
        linear, direct = c.traffic_model == _abi.TRAFFIC_LINEAR, c.ego_control == _abi.EGO_DIRECT
        family = "_linear" if linear else "_direct" if direct else ""
        if family:
            force_block = c.tune_block_kernel == 1 or n > 64
        else:
            force_block = c.tune_block_kernel == 1 or (c.tune_block_kernel == 0 and n > 128)
        nw = (n + 63) // 64
        if n <= 64 and not force_block:
            full_scan = not (c.flags & _abi.C_EGO_ONLY_COLLISIONS)
            stem, args = "hwy_{}_wave" + family + "_kernel", f"{w}, {'true' if full_scan else 'false'}"
        elif not family and 64 < n <= 256 and c.obs_type == _abi.OBS_KINEMATICS and not force_block:
            stem, args = "hwy_{}_wide_kernel", f"{nw}, {2 if nw == 2 else 1}"
        else:
            stem, args = "hwy_{}" + family + "_kernel", f"{nw}, {w}"
    return tuple(f"hwy::{stem.format(stage)}<{args}>" for stage in ("step", "rollout"))


def default_waves_per_eu(d: dict, kw: dict, num_envs: int, cus: int = 256) -> int:
    """hwy_create's own choice (csrc/hwy_engine.hip) for an untuned configuration on a part with `cus` compute units."""
    c = _abi.make_config(d, num_envs, **kw)
    if c.scenario == _abi.SCENARIO_INTERSECTION:
        helpers = c.num_vehicles <= 32 and not c.tune_ix_no_helpers
        return 3 if (num_envs > 2048 and not helpers) else 2
    if c.scenario != _abi.SCENARIO_HIGHWAY:
        return 4
    return 4 if num_envs * ((c.num_vehicles + 63) // 64) > 3 * 4 * cus else 3


# --------------------------------------------------------------------------- one build against another, bit for bit

def make_engine(backend: str, d: dict, kw: dict, E: int):
    from tests.families_util import make_engine as family_engine
    return family_engine(backend, _abi.make_config(d, E, **kw))


def reset_for_comparison(eng, d: dict, seeds, base_seed: int) -> None:
    """The device reset and the auto-reset every engine of one comparison gets: the same seeds, the same spawn arguments."""
    spawn = {"ego_spacing": float(d.get("ego_spacing", 2.0)), "vehicles_density": float(d.get("vehicles_density", 1.0))}
    eng.reset(seeds=np.asarray(seeds, np.uint64), **spawn)
    eng.set_autoreset(True, base_seed=base_seed, **spawn)


OUTPUTS = ("obs", "reward", "terminated", "truncated", "info speed", "info crashed")


def _planes(out) -> tuple:
    obs, reward, term, trunc, info = out
    return obs, reward, term, trunc, info["speed"], info["crashed"]


def _assert_outputs_equal(got, want, what: str) -> None:
    for name, a, b in zip(OUTPUTS, _planes(got), _planes(want)):
        assert a.shape == b.shape and a.size > 0, f"{what}: {name} {a.shape} / {b.shape}"
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: {name}")


def extras(eng) -> dict:
    """What an engine keeps beside its state planes: the Linear family's drawn parameters, a direct-control ego's stored action."""
    out = {}
    if eng.cfg.traffic_model == _abi.TRAFFIC_LINEAR:
        out["behavior"] = np.array(eng.get_behavior())
    if eng.cfg.ego_control == _abi.EGO_DIRECT:
        out["ctl_accel"], out["ctl_steer"] = (np.array(a) for a in eng.get_controls())
    return out


def _shape_library(eng):
    """The library whose launch layer runs an engine's launches: the emulation's unit of the engine's family, or the product's."""
    if hasattr(eng, "family"):
        from tests.emu import emu
        return emu.lib(eng.family)
    from highwayenv_amd import _lib
    return _lib.load()


def last_step_shape(eng) -> int:
    """hwy_last_step_shape() of the library behind `eng`: highwayenv_amd.engine.last_step_shape() on the product."""
    if hasattr(eng, "family"):
        return int(_shape_library(eng).hwy_last_step_shape())
    from highwayenv_amd import engine
    return engine.last_step_shape()


def assert_launched_shape(eng, rollout: bool, what: str) -> None:
    """The launch `eng` just made -- a full step() with auto-reset on (reset_for_comparison), or a rollout() -- ran the kernel
    step_shape() / launched() name for its configuration: the table cannot say one kernel while another runs.  The report is that
    of the straight-road families' launch layer; a road-network or intersection launch leaves it alone, and nothing is asserted."""
    if eng.cfg.scenario != _abi.SCENARIO_HIGHWAY:
        return
    enabled = _shape_library(eng).hwy_step_shapes(-1) == 1
    want = 0 if rollout or not enabled else step_shape_of_config(eng.cfg)
    got = last_step_shape(eng)
    assert got == want, f"{what}: the launch ran shape {got}, tests/variants_util.py: step_shape() says {want}"


def assert_builds_identical(ref, others: dict, K: int, seed: int = 5) -> int:
    """`ref` and every engine of `others` ({label: engine}; all reset alike by the caller: reset_for_comparison) take the same
    random actions through K calls of step() and then one rollout() of K more steps.  Every output of every step, the state
    afterwards and the engines' extras must be EQUAL, array_equal, on each of `others` against `ref`; an engine that counts them
    must have stored no non-finite value; every launch must have run the kernel the table names (assert_launched_shape).  Returns
    the number of episodes that ended on `ref` (each one an auto-reset inside a launch)."""
    assert others, "nothing to compare"
    cfg = ref.cfg
    E, A = cfg.num_envs, cfg.num_agents
    acts = np.random.default_rng(seed).integers(0, _abi.num_actions(cfg), size=(2 * K, E, A)).astype(np.int32)
    start = ref.get_state()
    for label, eng in others.items():
        assert (eng.cfg.num_envs, eng.cfg.num_vehicles, eng.cfg.num_agents) == (E, cfg.num_vehicles, A), label
        st = eng.get_state()
        for f in start:
            np.testing.assert_array_equal(st[f], start[f], err_msg=f"{label}: state {f} after the reset")
    n_done = 0
    for k in range(K):
        want = ref.step(acts[k])
        assert_launched_shape(ref, False, f"default: step {k}")
        n_done += int((want[2] | want[3]).sum())
        for label, eng in others.items():
            got = eng.step(acts[k])
            assert_launched_shape(eng, False, f"{label}: step {k}")
            _assert_outputs_equal(got, want, f"{label}: step {k}")
    want = ref.rollout(acts[K:])
    assert_launched_shape(ref, True, "default: rollout")
    assert want[0].shape[0] == K
    n_done += int((want[2] | want[3]).sum())
    for label, eng in others.items():
        got = eng.rollout(acts[K:])
        assert_launched_shape(eng, True, f"{label}: rollout")
        _assert_outputs_equal(got, want, f"{label}: rollout")
    want_state, want_extras = ref.get_state(), extras(ref)
    for label, eng in others.items():
        st, ex = eng.get_state(), extras(eng)
        assert set(st) == set(want_state) and set(ex) == set(want_extras), label
        for f in want_state:
            np.testing.assert_array_equal(st[f], want_state[f], err_msg=f"{label}: state {f}")
        for f in want_extras:
            np.testing.assert_array_equal(ex[f], want_extras[f], err_msg=f"{label}: {f}")
    for label, eng in {"default": ref, **others}.items():
        if hasattr(eng, "counters"):  # (the product; the emulation keeps no counters)
            assert eng.counters()["nonfinite_stores"] == 0, label
    return n_done


def compare_row(backend: str, d: dict, kw: dict, tunings: dict, E: int, K: int, seed: int = 5) -> int:
    """An untuned engine of the row against one engine per entry of `tunings` ({label: tuning knobs}), all with the same device
    reset.  Returns the number of episodes that ended (assert_builds_identical)."""
    seeds = 1000 * seed + np.arange(E)
    ref = make_engine(backend, d, kw, E)
    others = {label: make_engine(backend, d, with_tuning(kw, **knobs), E) for label, knobs in tunings.items()}
    try:
        for eng in (ref, *others.values()):
            reset_for_comparison(eng, d, seeds, base_seed=77 + seed)
        return assert_builds_identical(ref, others, K, seed)
    finally:
        for eng in (ref, *others.values()):
            eng.close()
