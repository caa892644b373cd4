"""Host reset (highwayenv_amd/spawn.py) against the reference's reset(seed=s) states."""
import numpy as np
import pytest

from highwayenv_amd import _abi, spawn
from oracle import ref_stub
from tests.golden_util import ALL, Golden


@pytest.mark.parametrize("name", ALL)
def test_spawn_matches_reference_reset(name):
    g = Golden(name)
    cfg = _abi.make_config(g.config, g.E, fast=g.fast)
    st = spawn.spawn_reference_stream(cfg, g.seeds, g.config["ego_spacing"], g.config["vehicles_density"],
                                      g.config["initial_lane_id"])
    want = g.state("init")
    for k in ["lane", "target_lane", "flags", "speed_index"]:
        np.testing.assert_array_equal(st[k], want[k], err_msg=k)
    for k in ["x", "y", "heading", "speed", "target_speed", "timer", "delta"]:
        np.testing.assert_allclose(st[k], want[k], rtol=0, atol=1e-12, err_msg=k)


def test_agent_indices_multi_agent():
    # HighwayEnv._create_vehicles with near_split(10, 3) = [4, 3, 3]
    assert _abi.agent_indices(10, 3) == [0, 5, 9]
    assert _abi.agent_indices(50, 1) == [0]


@pytest.mark.reference
@pytest.mark.skipif(not ref_stub.reference_available(), reason="needs the reference package")
@pytest.mark.parametrize("lanes", [1, 6])
@pytest.mark.parametrize("vehicles_count", [64, 128, 255])
def test_spawn_matches_live_reference_reset_at_large_sizes(vehicles_count, lanes):
    """The committed fixtures stop at 101 vehicles; the device spawns are held to ``spawn_from_draws`` up to N = 256
    (tests/test_spawn_paths.py).  Here the rule itself meets the unmodified reference's ``reset(seed=...)`` at the sizes where the
    kernels change path, on one and on six lanes: discrete planes exact, the others bit for bit."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden.py")
    spec = importlib.util.spec_from_file_location("make_golden", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)   # (installs the gymnasium / pygame stand-ins of oracle/ref_stub.py, imports the reference)
    ref_stub.restore_class_defaults()
    user = {"vehicles_count": vehicles_count, "lanes_count": lanes}
    seeds = [5, 2**31 - 1]
    cfg_d = dict(_abi.highway_default_config(), **user)
    cfg = _abi.make_config(cfg_d, len(seeds), fast=False)
    st = spawn.spawn_reference_stream(cfg, seeds, cfg_d["ego_spacing"], cfg_d["vehicles_density"], cfg_d["initial_lane_id"])
    env = gen.HighwayEnv(config=user)
    for e, seed in enumerate(seeds):
        env.reset(seed=seed)
        want = gen.dump_state(env)
        assert want["x"].shape == (vehicles_count + 1,)
        ctrl = want["controlled"] != 0
        for k in ["lane", "target_lane"]:
            np.testing.assert_array_equal(st[k][e], want[k], err_msg=k)
        np.testing.assert_array_equal(st["speed_index"][e][ctrl], want["speed_index"][ctrl])
        np.testing.assert_array_equal((st["flags"][e] & _abi.F_CONTROLLED) != 0, ctrl)
        np.testing.assert_array_equal((st["flags"][e] & _abi.F_CHECK_COLLISIONS) != 0, want["check_collisions"] != 0)
        for k in ["x", "y", "heading", "speed", "target_speed"]:
            np.testing.assert_array_equal(st[k][e], want[k], err_msg=k)
        for k in ["timer", "delta"]:   # (an MDPVehicle has neither)
            np.testing.assert_array_equal(st[k][e][~ctrl], want[k][~ctrl], err_msg=k)
        assert st["x"][e].max() < cfg.road_length
