"""Host side of the parking scenario (highwayenv_amd/parking.py): the host reset against the reference's recorded rule, what is
out of scope raises before the device is touched, spaces, registry, the C entry points' own refusals.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from highwayenv_amd import parking

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parking")


def test_host_reset_is_the_reference_rule_for_256_seeds():
    with np.load(os.path.join(GOLDEN, "reset_rule.npz")) as z:
        want = {k: z[k] for k in z.files}
    n = len(want["heading"])
    st = parking.spawn_reference_stream(26, [np.random.default_rng(s) for s in range(n)])
    assert np.array_equal(st["heading"], want["heading"]) and np.array_equal(st["goal"], want["goal"])
    assert np.array_equal(st["order"], want["order"])
    # the closest-lane rule itself (the device reset's restatement leans on it): heading -> the ego's spot, both columns met
    assert [parking.closest_spot(h) for h in want["heading"]] == list(want["ego_spot"]) and set(want["ego_spot"]) == {6, 20}
    few = parking.spawn_reference_stream(3, [np.random.default_rng(s) for s in range(8)])  # fewer vehicles: a prefix of the draws
    assert np.array_equal(few["order"][:, :3], want["order"][:8, :3]) and not few["order"][:, 3:].any()


@pytest.mark.parametrize("change", [
    {"controlled_vehicles": 2}, {"vehicles_count": 27}, {"vehicles_count": -1}, {"policy_frequency": 2}, {"simulation_frequency": 32, "policy_frequency": 2},
    {"observation": {"type": "Kinematics"}}, {"observation": {"type": "GrayscaleObservation"}},
    {"observation": {"features": ["x", "y", "vx", "vy", "sin_h", "cos_h"]}}, {"observation": {"vehicles_count": 3}},
    {"action": {"type": "DiscreteMetaAction"}}, {"action": {"dynamical": True}}, {"action": {"speed_range": [0, 10]}},
    {"action": {"clip": False}}, {"action": {"lateral": False}}, {"action": {"longitudinal": False}},
    {"action": {"steering_range": [-1.2, 1.2]}},
])
def test_out_of_scope_configs_raise_before_the_device(change, monkeypatch):
    monkeypatch.setattr(parking, "ParkEngine", lambda *a, **k: pytest.fail("the device was touched"))
    with pytest.raises(NotImplementedError):
        parking.BatchedParkingEnv(change, num_envs=2)
    with pytest.raises(NotImplementedError):
        parking.BatchedParkingEnv(render_mode="human")
    env = parking.BatchedParkingEnv(num_envs=2)
    with pytest.raises(NotImplementedError):
        env.compute_reward(np.zeros(6), np.zeros(6), {}, p=1.0)
    from highwayenv_amd.vector import HighwayVectorEnv
    with pytest.raises(NotImplementedError):
        HighwayVectorEnv("parking-v0", 2, autoreset_mode="SameStep")


def test_config_quirks_and_spaces():
    env = parking.BatchedParkingEnv({"steering_range": 0.1, "action": {"acceleration_range": [-3.3, 2.1]}}, num_envs=3)
    c = env._pcfg
    assert list(c.steering_range) == [-np.pi / 4, np.pi / 4]  # the top-level key is never read by ContinuousAction
    assert list(c.acceleration_range) == [-3.3, 2.1] and c.frames == 3 and c.dt == 1 / 15 and c.policy_dt == 1 / 5
    assert parking.BatchedParkingEnvActionRepeat(num_envs=1)._pcfg.frames == 15
    assert parking.BatchedParkingEnvParkedVehicles(num_envs=1)._pcfg.vehicles_count == 10
    assert set(env.single_observation_space) == {"observation", "achieved_goal", "desired_goal"}
    assert all(tuple(env.single_observation_space[k].shape) == (6,) for k in env.single_observation_space)
    assert tuple(env.single_action_space.shape) == (2,) and env.single_action_space.dtype == np.float32
    one = {"observation": np.arange(6, dtype=np.float32)[None], "achieved_goal": np.zeros((1, 6), np.float32), "desired_goal": np.ones((1, 6), np.float32)}
    got = parking.ParkingEnv._one(one)  # the drop-in's observation: the reference's dict of float64 rows
    assert list(got) == ["observation", "achieved_goal", "desired_goal"] and got["observation"].dtype == np.float64 and got["observation"].shape == (6,)
    info = parking.ParkingEnv._one_info({"speed": np.ones(1), "crashed": np.zeros(1, bool), "is_success": np.ones(1, bool)})
    assert info["is_success"] is True and info["crashed"] is False


def test_registry_ids_resolve():
    from highwayenv_amd import envs
    from highwayenv_amd.vector import HighwayVectorEnv
    assert {k: (s.__name__, b.__name__) for k, (s, b) in parking.REGISTRY.items()} == {
        "parking-v0": ("ParkingEnv", "BatchedParkingEnv"), "parking-ActionRepeat-v0": ("ParkingEnvActionRepeat", "BatchedParkingEnvActionRepeat"),
        "parking-parked-v0": ("ParkingEnvParkedVehicles", "BatchedParkingEnvParkedVehicles")}
    assert not set(parking.REGISTRY) & set(envs.REGISTRY)
    for env_id, (single, batched) in parking.REGISTRY.items():
        assert issubclass(single, batched) and parking.is_parking_id("highwayenv_amd/" + env_id)
        vec = HighwayVectorEnv(env_id, 4)  # (the engine is created by reset(): none here)
        assert isinstance(vec, parking.ParkingVectorEnv) and vec.num_envs == 4 and vec.autoreset_mode == "NextStep"
        assert isinstance(vec.env, batched) and vec.env.autoreset and tuple(vec.single_action_space.shape) == (2,)


def test_c_entry_points_refuse_bad_configs_and_no_device():
    lib = parking.load()
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "..", "include", "hwy_park.h")).read()
    for name in parking.EXPORTS:
        assert hasattr(lib, name) and f"{name}(" in header, name
    good = parking.make_park_config(parking.parking_default_config(), 2)
    for field, value in [("struct_size", 8), ("num_envs", 0), ("vehicles_count", 27), ("frames", 16), ("frames", 0), ("dt", 0.0)]:
        cfg = parking.HwyParkConfig.from_buffer_copy(bytes(good))
        setattr(cfg, field, value)
        h = C.c_void_p()
        assert lib.hwy_park_create(C.byref(cfg), 0, None, C.byref(h)) == 1 and not h.value, field
        assert lib.hwy_park_last_error(None)
    bad = parking.HwyParkConfig.from_buffer_copy(bytes(good))
    bad.steering_range[1] = 1.2
    h = C.c_void_p()
    assert lib.hwy_park_create(C.byref(bad), 0, None, C.byref(h)) == 1 and b"pi/3" in lib.hwy_park_last_error(None)
    from highwayenv_amd import _lib
    if _lib.load().hwy_device_count() == 0:
        assert lib.hwy_park_create(C.byref(good), 0, None, C.byref(h)) == 4 and b"no CPU fallback" in lib.hwy_park_last_error(None)
