"""The C oracle against the unmodified reference on RANDOM configurations.

tests/test_oracle_golden*.py pin the oracle on 45 committed scenarios; here configurations and seeds are drawn at random from
the same spaces the engine-vs-oracle fuzz draws from (tests/test_fuzz_configs.py), the reference class is driven through
oracle/ref_stub.py by the committed fixture generators (tests/golden/make_golden*.py: run_scenario), and the oracle is held to
the SAME checks as on the fixtures: every recorded frame teacher-forced from the reference's own state at 1e-10 (flags / lane
indices / routes exact, impacts signed off the knife edge), and the observation / reward / terminated / truncated / info of
every policy step at 1e-6 / 1e-9 / exact.

The reference's traces of the default cases are committed under tests/golden/live (tests/golden/make_golden_live.py writes
them), together with the scenario each was drawn as: a case whose draw no longer matches its recording fails and asks for a
regeneration.  Cases beyond the recorded ones run the reference live where it is installed (oracle/ref_stub.py) and are
skipped elsewhere.

HWY_REF_FUZZ configurations per family (default 12: seconds per family in the default suite; the round's full run,
HWY_REF_FUZZ=240 under pytest-xdist, is recorded in profiles/r04_ref_fuzz.txt).  A configuration's seed is its number:
HWY_REF_FUZZ_FIRST continues where the last run ended."""
import importlib.util
import json
import os

import numpy as np
import pytest

from oracle import ref_stub
from tests import test_fuzz_configs as fz

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RECORDED = os.path.join(GOLDEN, "live")
RECORDED_CASES = 12   # cases 0 .. 11 of every family are committed under tests/golden/live
FIRST = int(os.environ.get("HWY_REF_FUZZ_FIRST", "0"))
CASES = range(FIRST, FIRST + int(os.environ.get("HWY_REF_FUZZ", "12")))
GENERATORS = {"highway": "make_golden.py", "merge": "make_golden_merge.py", "intersection": "make_golden_intersection.py"}
_mods = {}


def _generator(fname):
    if fname not in _mods:
        spec = importlib.util.spec_from_file_location(fname[:-3], os.path.join(GOLDEN, fname))
        _mods[fname] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_mods[fname])
    return _mods[fname]


def _user_config(cfg: dict, defaults: dict) -> dict:
    """The entries of a full config dict that differ from the product's defaults: what a user passes to the reference class."""
    return {k: v for k, v in cfg.items() if k not in defaults or defaults[k] != v}


def _highway_draw(case: int):
    """Case `case` of the highway family: the generator's scenario dict (the reference class by name, `cls`) and the full
    configuration drawn."""
    from highwayenv_amd import _abi
    rng = np.random.default_rng(61_000 + case)
    cfg, fast = fz.random_config(rng)
    while cfg["controlled_vehicles"] != 1:   # (the highway generator drives one agent; merge and intersection below drive several)
        cfg, fast = fz.random_config(rng)
    cfg["vehicles_count"] = min(cfg["vehicles_count"], 45)
    table = 5 if "longitudinal" not in cfg["action"] and "lateral" not in cfg["action"] else 3
    defaults = _abi.highway_fast_default_config() if fast else _abi.highway_default_config()
    sc = dict(name=f"live_highway_{case}", cls="HighwayEnvFast" if fast else "HighwayEnv", config=_user_config(cfg, defaults),
              seeds=[int(rng.integers(0, 2**31))], steps=int(rng.integers(3, 6)), action_seed=int(rng.integers(0, 2**31)),
              frames_for=1, n_actions=table)
    return sc, cfg


def highway_scenario(case: int) -> dict:
    return _highway_draw(case)[0]


def merge_scenario(case: int) -> dict:
    from highwayenv_amd import _abi, merge
    rng = np.random.default_rng(62_000 + case)
    generic = bool(rng.integers(4))   # merge-generic three times out of four, merge-v0 / -v1 otherwise
    if generic:
        cfg = fz.random_merge_config(rng)
        cfg["vehicles_count"] = min(cfg["vehicles_count"], 35)
        # (several controlled vehicles: the generator's subclass that makes the first A - 1 traffic vehicles MDPVehicles -- BASELINE
        #  config 5's extension, tests/golden/make_golden_merge.py -- everything that steps, observes and rewards is the reference's)
        cls = "MergeGenericMultiAgent" if cfg["controlled_vehicles"] > 1 else "MergeGenericEnv"
        user = _user_config(cfg, merge.merge_generic_default_config())
        oc = user.get("observation", {}).get("observation_config")
        if cfg["controlled_vehicles"] > 1 and oc and oc["type"] == "Kinematics":
            # KinematicObservation derives its default y range from the lanes beside the OBSERVER's lane at its first observation
            # (observation.py:214-227); the extension's agents 2..A are traffic vehicles that may start on b->c (one lane more than
            # a->b).  The product defines the extension with ONE range, the ego's: stated here explicitly,
            # like in the committed merge_ma4 fixtures
            L = cfg["lanes_count"]
            oc["features_range"] = {"x": [-200, 200], "y": [-4 * L, 4 * L], "vx": [-80, 80], "vy": [-80, 80]}
    else:
        connected = bool(rng.integers(2))
        cls = "ConnectedLaneMergeEnv" if connected else "MergeEnv"
        user = {}
    full = dict(merge.merge_generic_default_config() if generic else merge.merge_default_config(), **user)
    n_slots = int(_abi.make_config(full, 1, scenario="merge-generic" if generic else "merge").num_vehicles)  # (the product's slot count)
    return dict(name=f"live_merge_{case}", cls=cls, config=user, seeds=[int(rng.integers(0, 2**31))], steps=int(rng.integers(3, 6)),
                action_seed=int(rng.integers(0, 2**31)), frames_for=1, n_slots=n_slots)


def intersection_scenario(case: int) -> dict:
    from highwayenv_amd import intersection as hix
    rng = np.random.default_rng(63_000 + case)
    cfg = fz.random_intersection_config(rng)
    A = int(cfg["controlled_vehicles"])
    connected = bool(cfg.pop("neighbour_vehicles_connected_lanes", False))
    cfg.pop("max_vehicles", None)   # (an engine option: the reference's vehicle list is unbounded)
    user = _user_config(cfg, hix.intersection_default_config())
    if A > 1:
        connected = False   # (MultiAgentIntersectionEnv derives from IntersectionEnv)
        user["observation"] = {"type": "MultiAgentObservation", "observation_config": cfg["observation"]}
    return dict(name=f"live_intersection_{case}", config=user, seeds=[int(rng.integers(0, 2**31))], steps=int(rng.integers(3, 7)),
                action_seed=int(rng.integers(0, 2**31)), frames_for=1, n_slots=40, r_max=8,   # (destination == origin: a 6-lane U-turn route)
                **({"cls": "MultiAgentIntersectionEnv"} if A > 1 else {"cls": "ConnectedLaneIntersectionEnv"} if connected else {}))


SCENARIOS = {"highway": highway_scenario, "merge": merge_scenario, "intersection": intersection_scenario}


def scenario_json(sc: dict) -> str:
    return json.dumps(sc, sort_keys=True)


def run_live(family: str, sc: dict) -> dict:
    """The reference's trace of scenario `sc` (needs the reference package).  The merge family raises IndexError where the
    rejection-sampled spawn placed fewer traffic vehicles than there are agents to make of them."""
    gen = _generator(GENERATORS[family])
    if family != "intersection":   # (the highway and merge generators take the class itself)
        sc = dict(sc, cls=getattr(gen, sc["cls"]))
    return gen.run_scenario(sc)


def _trace(family: str, case: int) -> dict:
    """The reference's trace of case `case`: the committed recording, or -- beyond the recorded cases -- a live run."""
    sc = SCENARIOS[family](case)
    path = os.path.join(RECORDED, sc["name"] + ".npz")
    if os.path.exists(path):
        z = np.load(path)
        assert str(z["scenario_json"]) == scenario_json(sc), (
            f"{sc['name']}: the committed trace was recorded for another draw of this case; regenerate it with "
            f"`python tests/golden/make_golden_live.py {sc['name']}`")
        if "skipped" in z.files:
            pytest.skip(str(z["skipped"]))
        return {k: z[k] for k in z.files if k != "scenario_json"}
    assert case >= RECORDED_CASES, f"{path} is missing"
    if not ref_stub.reference_available():
        pytest.skip(f"case {case} is not recorded (cases 0 .. {RECORDED_CASES - 1} are): it needs the reference package")
    try:
        return run_live(family, sc)
    except IndexError:
        if family != "merge":
            raise
        pytest.skip("fewer traffic vehicles than controlled_vehicles - 1")


@pytest.mark.parametrize("case", CASES)
def test_random_highway_configuration(case):
    from tests.golden_util import Golden
    from tests.test_oracle_golden import check_free_running_steps, check_teacher_forced_frames
    sc, cfg = _highway_draw(case)
    data = _trace("highway", case)
    try:
        g = Golden(sc["name"], data=data)
        check_teacher_forced_frames(g)
        if cfg["observation"].get("order") != "shuffled" and cfg["observation"]["type"] == "Kinematics":
            check_free_running_steps(g)   # (3-5 steps from reset: obs / reward / done / info / state)
    except AssertionError as ex:
        raise AssertionError(f"{sc}\n{ex}") from ex


@pytest.mark.parametrize("case", CASES)
def test_random_merge_configuration(case):
    from tests.golden_util import GoldenMerge
    from tests.test_oracle_golden_merge import check_free_running_steps, check_teacher_forced_frames
    sc = merge_scenario(case)
    data = _trace("merge", case)
    try:
        g = GoldenMerge(sc["name"], data=data)
        check_teacher_forced_frames(g)
        if g.config["observation"].get("order", g.config["observation"].get("observation_config", {}).get("order")) != "shuffled":
            check_free_running_steps(g)
    except AssertionError as ex:
        raise AssertionError(f"{sc}\n{ex}") from ex


@pytest.mark.parametrize("case", CASES)
def test_random_intersection_configuration(case):
    from tests.golden_util import GoldenIntersection
    from tests.test_oracle_golden_intersection import check_steps_observation_reward_and_clear_spawn, check_teacher_forced_frames
    sc = intersection_scenario(case)
    data = _trace("intersection", case)
    try:
        g = GoldenIntersection(sc["name"], data=data)
        check_teacher_forced_frames(g, coverage=False)
        check_steps_observation_reward_and_clear_spawn(g, coverage=False)
    except AssertionError as ex:
        raise AssertionError(f"{sc}\n{ex}") from ex
