"""Direct ego control (``DiscreteAction``) on the host side (no GPU): the config it is accepted in and the axis tables it
yields, the errors, the spaces, the single-environment drop-in, and the fixtures of tests/golden/control against their manifest
and, where the reference is installed, against the reference itself."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

from highwayenv_amd import _abi, envs, spawn
from oracle import ref_stub
from tests.control_util import CONTROL_DIR, FIXTURES, ControlGolden


def _cfg(fast=True, **action):
    d = _abi.highway_fast_default_config() if fast else _abi.highway_default_config()
    d["action"] = dict({"type": "DiscreteAction"}, **action)
    return d


@pytest.mark.parametrize("name", FIXTURES)
def test_axis_tables_are_the_reference_float32_values_bit_for_bit(name):
    """Action id a means (accel_axis[a // n_steer], steer_axis[a % n_steer]): for every id the pair equals what the reference's
    get_action mapped the float32 table entry to (recorded in the fixture), bit for bit."""
    g = ControlGolden(name)
    c = g.hwy_config()
    assert c.ego_control == _abi.EGO_DIRECT
    want_a, want_s = g.z["axis_accel"], g.z["axis_steer"]
    assert _abi.num_actions(c) == c.n_accel * c.n_steer == len(want_a) == len(g.z["all_actions"])
    assert g.z["all_actions"].dtype == np.float32
    got_a = np.array([c.accel_axis[a // c.n_steer] for a in range(len(want_a))])
    got_s = np.array([c.steer_axis[a % c.n_steer] for a in range(len(want_a))])
    np.testing.assert_array_equal(got_a, want_a)
    np.testing.assert_array_equal(got_s, want_s)


def test_lmap_runs_in_float32():
    """utils.lmap of a float32 table entry stays float32 under NumPy 2: every axis value is a float32 number, and where the f64
    evaluation of the same expression is not one (the inner points of a 4-point axis, +-1/3) the two differ."""
    accel, steer = _abi.direct_action_axes({"type": "DiscreteAction", "actions_per_axis": 4})
    for v in accel + steer:
        assert v == float(np.float32(v))
    f64 = -np.pi / 4 + (np.linspace(-1.0, 1.0, 4) - -1) * (np.pi / 4 - -np.pi / 4) / (1 - -1)
    assert steer[1] != f64[1] and abs(steer[1] - f64[1]) < 1e-7
    x = np.float32(-0.7)  # the issue's example: float32(-0.5497787), not -0.5497787143782138
    assert float(-np.pi / 4 + (x - -1) * (np.pi / 4 - -np.pi / 4) / (1 - -1)) == -0.5497786998748779


def test_defaults_and_single_axis_tables():
    c = _abi.make_config(_cfg(), 2, fast=True)
    assert (c.n_accel, c.n_steer) == (3, 3)
    assert list(c.accel_axis[:3]) == [-5.0, 0.0, 5.0]
    assert list(c.steer_axis[:3]) == [float(np.float32(-np.pi / 4)), 0.0, float(np.float32(np.pi / 4))]
    c = _abi.make_config(_cfg(lateral=False, actions_per_axis=4), 2, fast=True)
    assert (c.n_accel, c.n_steer, c.steer_axis[0]) == (4, 1, 0.0) and _abi.num_actions(c) == 4
    c = _abi.make_config(_cfg(longitudinal=False), 2, fast=True)
    assert (c.n_accel, c.n_steer, c.accel_axis[0]) == (1, 3, 0.0) and _abi.num_actions(c) == 3
    # the meta-action config is what it was (ABI v7 appends the fields: zeros)
    m = _abi.make_config(_abi.highway_fast_default_config(), 2, fast=True)
    assert (m.ego_control, m.n_accel, m.n_steer) == (_abi.EGO_META, 0, 0) and _abi.num_actions(m) == 5


def test_config_errors():
    with pytest.raises(ValueError):  # action.py:108-111
        _abi.make_config(_cfg(longitudinal=False, lateral=False), 2)
    with pytest.raises(NotImplementedError):
        _abi.make_config(_cfg(dynamical=True), 2)
    with pytest.raises(ValueError):  # beyond the kernels' tan (Vehicle.MAX_STEERING_ANGLE)
        _abi.make_config(_cfg(steering_range=[-1.2, 1.2]), 2)
    with pytest.raises(NotImplementedError):
        _abi.make_config(_cfg(actions_per_axis=17), 2)
    with pytest.raises(ValueError):
        _abi.make_config(_cfg(actions_per_axis=0), 2)
    with pytest.raises(NotImplementedError):  # Linear-family traffic with a direct-control ego: out of scope
        _abi.make_config(dict(_cfg(), other_vehicles_type="highway_env.vehicle.behavior.LinearVehicle"), 2)
    from highwayenv_amd import intersection, merge
    with pytest.raises(NotImplementedError):
        _abi.make_config(dict(merge.merge_default_config(), action={"type": "DiscreteAction"}), 2, scenario="merge")
    with pytest.raises(NotImplementedError):
        _abi.make_config(dict(intersection.intersection_default_config(), action={"type": "DiscreteAction"}), 2,
                         scenario="intersection")
    with pytest.raises(NotImplementedError):  # ContinuousAction stays rejected, with its present error
        _abi.make_config(dict(_abi.highway_default_config(), action={"type": "ContinuousAction"}), 2)


def test_spaces():
    e = envs.BatchedHighwayEnvFast(_cfg(actions_per_axis=5), num_envs=3)
    assert e.single_action_space.n == 25
    e = envs.BatchedHighwayEnvFast(_cfg(lateral=False), num_envs=3)
    assert e.single_action_space.n == 3
    ma = dict(_cfg(), controlled_vehicles=2, action={"type": "MultiAgentAction", "action_config": {"type": "DiscreteAction"}},
              observation={"type": "MultiAgentObservation", "observation_config": {"type": "Kinematics"}})
    e = envs.BatchedHighwayEnvFast(ma, num_envs=3)
    assert e._hcfg.num_agents == 2 and e.single_action_space.n == 9 and e.single_observation_shape == (2, 5, 5)


@pytest.mark.parametrize("name", FIXTURES)
def test_host_spawn_gives_the_ego_the_state_it_gives_it_today(name):
    """Same draws as the meta-action spawn (Vehicle.create_random first, then the class copy): positions, speeds, lanes of every
    vehicle are the reference's, bit for bit."""
    g = ControlGolden(name)
    st = spawn.spawn_reference_stream(g.hwy_config(), g.seeds, g.config["ego_spacing"], g.config["vehicles_density"])
    want = g.state("init")
    for k in ["x", "y", "heading", "speed", "lane", "flags"]:
        np.testing.assert_array_equal(st[k], want[k], err_msg=k)
    other = (want["flags"] & _abi.F_CONTROLLED) == 0
    for k in ["timer", "delta", "target_speed"]:
        np.testing.assert_array_equal(st[k][other], want[k][other], err_msg=k)


class _EmuHighwayEnvFast(envs.HighwayEnvFast):
    @staticmethod
    def _engine_factory(cfg, device, stream):
        from tests.emu.emu import EmuEngine
        return EmuEngine(cfg)


def test_single_env_drop_in_replays_direct_fast_env0():
    """gym-style use on the emulation of the kernels: reset(seed) spawns on the reference's stream, step(int) returns the
    reference's observation, reward, terminated; env.vehicle is a plain Vehicle's view; a bad id raises IndexError."""
    g = ControlGolden("direct_fast")
    env = _EmuHighwayEnvFast(dict(g.config))
    obs, info = env.reset(seed=int(g.seeds[0]))
    np.testing.assert_allclose(obs, g.z["obs0"][0, 0], rtol=0, atol=1e-6)
    assert env.action_space.n == 9
    v = env.vehicle
    assert v.controlled and not hasattr(v, "target_lane_index") and not hasattr(v, "speed_index") and not hasattr(v, "target_speed")
    assert hasattr(env.road().vehicles[1], "target_lane_index")
    for t in range(g.steps):
        obs, reward, term, trunc, info = env.step(int(g.actions[t, 0, 0]))
        np.testing.assert_allclose(obs, g.z["obs"][t, 0, 0], rtol=0, atol=1e-6, err_msg=f"step {t}")
        assert abs(reward - g.z["reward"][t, 0]) <= 1e-9 and term == bool(g.z["terminated"][t, 0])
        assert info["rewards"]["right_lane_reward"] == env.vehicle.lane_index[2] / 3
        assert info["speed"] == g.z["step_speed"][t, 0, 0]
        if term:
            break
    for bad in (9, -1):
        with pytest.raises(IndexError):
            env.step(bad)


def _digest(data):  # (make_golden_control.digest restated: the generator imports the reference)
    import hashlib
    h = hashlib.sha256()
    for k in sorted(data.files):
        a = data[k]
        h.update(k.encode())
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_fixture_digests_match_the_manifest():
    """Every file under tests/golden/control is accounted for: the fixtures by the digest of their arrays, the rest by name."""
    manifest = json.load(open(os.path.join(CONTROL_DIR, "MANIFEST.json")))
    assert sorted(manifest) == sorted(FIXTURES)
    files = sorted(f for f in os.listdir(CONTROL_DIR) if not f.startswith("__"))
    assert files == sorted([n + ".npz" for n in FIXTURES] + ["MANIFEST.json", "README.md", "make_golden_control.py"])
    for name in FIXTURES:
        path = os.path.join(CONTROL_DIR, name + ".npz")
        assert os.path.getsize(path) <= 300 * 1024, name
        with np.load(path) as z:
            assert _digest(z) == manifest[name], name


def test_fixtures_record_a_plain_vehicle_ego():
    for name in FIXTURES:
        g = ControlGolden(name)
        z, agents = g.z, list(g.hwy_config().agent_index[:g.A])
        for prefix in ("init", "step") + (("frame",) if g.frames_for else ()):
            assert (z[prefix + "_controlled"][..., agents] == 1).all() and z[prefix + "_controlled"].sum(-1).max() == g.A
            assert (z[prefix + "_target_speed"][..., agents] == 0.0).all()
            assert (z[prefix + "_speed_index"][..., agents] == -1).all()
            np.testing.assert_array_equal(z[prefix + "_target_lane"][..., agents], z[prefix + "_lane"][..., agents])
        assert not z["init_act_accel"].any() and not z["init_act_steering"].any()  # Vehicle.__init__


@pytest.mark.reference
@pytest.mark.skipif(not ref_stub.reference_available(), reason="needs the reference package")
@pytest.mark.parametrize("name", FIXTURES)
def test_env0_regenerates_bit_for_bit(name):
    spec = importlib.util.spec_from_file_location("make_golden_control", os.path.join(CONTROL_DIR, "make_golden_control.py"))
    mgc = sys.modules.get("make_golden_control")
    if mgc is None:
        mgc = importlib.util.module_from_spec(spec)
        sys.modules["make_golden_control"] = mgc
        spec.loader.exec_module(mgc)
    sc = dict(next(s for s in mgc.SCENARIOS if s["name"] == name))
    got = mgc.run(sc, only_envs={0})
    with np.load(os.path.join(CONTROL_DIR, name + ".npz")) as z:
        for k in z.files:
            a = z[k]
            if k.startswith(("init_", "obs0")):
                np.testing.assert_array_equal(got[k][0], a[0], err_msg=k)
            elif k.startswith(("step_", "frame_")) or k in ("obs", "reward", "terminated", "truncated"):
                np.testing.assert_array_equal(got[k][:, 0], a[:, 0], err_msg=k)
            elif k not in ("meta", "seeds"):
                np.testing.assert_array_equal(got[k], a, err_msg=k)
