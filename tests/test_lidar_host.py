"""LidarObservation on the host side (no GPU): the configs it is accepted in, the fields it fills, the errors, the spaces and
shapes, the ABI layout, the gym-style drop-in on the emulated kernels, and the fixtures of tests/golden/lidar against their
manifest and, where the reference is installed, against the reference itself."""
import ctypes as C
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

from highwayenv_amd import _abi, _lib, envs
from oracle import ref_stub
from tests.lidar_util import FIXTURES, LIDAR_DIR, RUNS, LidarGolden

LINEAR = "highway_env.vehicle.behavior.LinearVehicle"


def _cfg(fast=True, **obs):
    d = _abi.highway_fast_default_config() if fast else _abi.highway_default_config()
    d["observation"] = dict({"type": "LidarObservation"}, **obs)
    return d


def test_defaults_and_fields():
    c = _abi.make_config(_cfg(), 3, fast=True)  # LidarObservation.__init__: cells 16, maximum_range 60, normalize True
    assert c.abi_version == _abi.HWY_ABI_VERSION == 8 and _abi.OBS_LIDAR == 2 and _abi.HWY_MAX_LIDAR_CELLS == 64
    assert (c.obs_type, c.lidar_cells, c.lidar_max_range, c.lidar_normalize) == (_abi.OBS_LIDAR, 16, 60.0, 1)
    assert _abi.obs_shape(c) == (16, 2)
    c = _abi.make_config(_cfg(cells=64, maximum_range=35, normalize=False), 3, fast=True)
    assert (c.lidar_cells, c.lidar_max_range, c.lidar_normalize) == (64, 35.0, 0) and _abi.obs_shape(c) == (64, 2)
    # the other observation types leave the appended fields at zero
    k = _abi.make_config(_abi.highway_fast_default_config(), 3, fast=True)
    assert (k.obs_type, k.lidar_cells, k.lidar_max_range, k.lidar_normalize) == (_abi.OBS_KINEMATICS, 0, 0.0, 0)


def test_every_straight_road_family_takes_it():
    ma = dict(_cfg(cells=24), controlled_vehicles=2,
              observation={"type": "MultiAgentObservation", "observation_config": {"type": "LidarObservation", "cells": 24}},
              action={"type": "MultiAgentAction", "action_config": {"type": "DiscreteMetaAction"}})
    c = _abi.make_config(ma, 2, fast=True)
    assert (c.num_agents, c.obs_type, _abi.obs_shape(c)) == (2, _abi.OBS_LIDAR, (24, 2))
    c = _abi.make_config(dict(_cfg(), other_vehicles_type=LINEAR), 2, fast=True)
    assert (c.traffic_model, c.obs_type) == (_abi.TRAFFIC_LINEAR, _abi.OBS_LIDAR)
    c = _abi.make_config(dict(_cfg(), action={"type": "DiscreteAction"}), 2, fast=True)
    assert (c.ego_control, c.obs_type) == (_abi.EGO_DIRECT, _abi.OBS_LIDAR)
    c = _abi.make_config(_cfg(fast=False), 2)
    assert c.obs_type == _abi.OBS_LIDAR and not (c.flags & _abi.C_EGO_ONLY_COLLISIONS)


def test_config_errors():
    from highwayenv_amd import intersection, merge
    lidar = {"type": "LidarObservation"}
    with pytest.raises(NotImplementedError):
        _abi.make_config(dict(merge.merge_default_config(), observation=lidar), 2, scenario="merge")
    with pytest.raises(NotImplementedError):
        _abi.make_config(dict(merge.merge_default_config(), observation=lidar), 2, scenario="merge-generic")
    with pytest.raises(NotImplementedError):
        _abi.make_config(dict(intersection.intersection_default_config(), observation=lidar), 2, scenario="intersection")
    with pytest.raises(NotImplementedError):
        _abi.make_config(_cfg(cells=65), 2)
    _abi.make_config(_cfg(cells=64), 2)
    with pytest.raises(ValueError):
        _abi.make_config(_cfg(cells=0), 2)
    with pytest.raises(ValueError):
        _abi.make_config(_cfg(maximum_range=0), 2)
    with pytest.raises(NotImplementedError):  # the other observation types stay where they were
        _abi.make_config(dict(_abi.highway_default_config(), observation={"type": "TimeToCollision"}), 2)
    with pytest.raises(ValueError):
        _abi.make_config(dict(_abi.highway_default_config(), observation={"type": "Sonar"}), 2)


def test_spaces_and_shapes():
    for kw, high in ((dict(), 1.0), (dict(normalize=False, maximum_range=35, cells=64), 35.0)):
        e = envs.BatchedHighwayEnvFast(_cfg(**kw), num_envs=3)
        cells = kw.get("cells", 16)
        sp = e.single_observation_space
        assert e.single_observation_shape == tuple(sp.shape) == (cells, 2) and np.dtype(sp.dtype) == np.float32
        assert np.all(np.asarray(sp.low) == -high) and np.all(np.asarray(sp.high) == high)
    ma = dict(_cfg(cells=8), controlled_vehicles=2,
              observation={"type": "MultiAgentObservation", "observation_config": {"type": "LidarObservation", "cells": 8}},
              action={"type": "MultiAgentAction", "action_config": {"type": "DiscreteMetaAction"}})
    e = envs.BatchedHighwayEnvFast(ma, num_envs=3)
    assert e.single_observation_shape == (2, 8, 2) and e.single_action_space.n == 5
    with pytest.raises(NotImplementedError):
        envs.BatchedMergeEnv({"observation": {"type": "LidarObservation"}}, num_envs=2)
    with pytest.raises(NotImplementedError):
        envs.BatchedIntersectionEnv({"observation": {"type": "LidarObservation"}}, num_envs=2)


def test_abi_struct_size_against_sizeof():
    """hwy_config as the C compilers lay it out (the engine library and the emulator's translation unit) against the ctypes
    mirror; the appended fields are the last 16 bytes."""
    from tests.emu import emu
    assert emu.lib("lidar").emu_lidar_config_size() == C.sizeof(_abi.HwyConfig)
    lib = _lib.load()
    assert lib.hwy_abi_version() == 8 and lib.hwy_config_size() == C.sizeof(_abi.HwyConfig)
    assert _abi.HwyConfig.lidar_cells.offset == C.sizeof(_abi.HwyConfig) - 16
    assert _abi.HwyConfig.lidar_max_range.offset == C.sizeof(_abi.HwyConfig) - 8
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hwy_engine.h")).read()
    assert "#define HWY_ABI_VERSION 8" in header and "HWY_OBS_LIDAR = 2" in header and "#define HWY_MAX_LIDAR_CELLS 64" in header
    assert "hwy_lidar_kernel" in lib_kernel_names()


def lib_kernel_names() -> str:
    from highwayenv_amd import build
    return " ".join(build.kernel_resources())


def test_create_rejects_bad_lidar_fields_before_it_needs_a_gpu():
    """hwy_create validates before it looks for a device: INVALID_ARG with its message, with or without a GPU."""
    lib = _lib.load()

    def create(c):
        h = C.c_void_p()
        rc = lib.hwy_create(C.byref(c), 0, None, C.byref(h))
        if rc == 0:
            lib.hwy_destroy(h)
        return rc, lib.hwy_last_error(None).decode()

    good = _abi.make_config(_cfg(), 2, fast=True)
    for field, value, word in (("lidar_cells", 0, "lidar_cells"), ("lidar_cells", 65, "lidar_cells"), ("lidar_max_range", 0.0, "lidar_max_range"),
                               ("lidar_max_range", float("inf"), "lidar_max_range"), ("lidar_normalize", 2, "lidar_normalize")):
        c = _abi.HwyConfig.from_buffer_copy(bytes(good))
        setattr(c, field, value)
        rc, msg = create(c)
        assert rc == _abi.HWY_ERR_INVALID_ARG and word in msg, (field, value, rc, msg)
    from highwayenv_amd import merge
    c = _abi.make_config(merge.merge_default_config(), 2, scenario="merge")
    c.obs_type, c.lidar_cells, c.lidar_max_range = _abi.OBS_LIDAR, 16, 60.0
    rc, msg = create(c)
    assert rc == _abi.HWY_ERR_INVALID_ARG and "highway scenario only" in msg
    rc, msg = create(good)
    assert rc in (_abi.HWY_OK, _abi.HWY_ERR_NO_DEVICE), msg


class _EmuHighwayEnvFast(envs.HighwayEnvFast):
    @staticmethod
    def _engine_factory(cfg, device, stream):
        from tests.emu.emu import EmuEngine
        return EmuEngine(cfg)


def test_single_env_drop_in_replays_lidar_fast_env0():
    """gym-style use on the emulation of the kernels: reset(seed) spawns on the reference's stream and returns its lidar
    observation, step(int) the observation / reward / terminated of the reference's run."""
    g = LidarGolden("lidar_fast")
    env = _EmuHighwayEnvFast(dict(g.config))
    obs, info = env.reset(seed=int(g.seeds[0]))
    assert obs.shape == (16, 2) and obs.dtype == np.float32
    np.testing.assert_allclose(obs, g.z["obs0"][0, 0], rtol=0, atol=1e-6)
    for t in range(g.steps):
        obs, reward, term, trunc, info = env.step(int(g.actions[t, 0, 0]))
        np.testing.assert_allclose(obs, g.z["obs"][t, 0, 0], rtol=0, atol=1e-6, err_msg=f"step {t}")
        assert abs(reward - g.z["reward"][t, 0]) <= 1e-9 and term == bool(g.z["terminated"][t, 0])
        assert env.observation_space.contains(obs)
        if term:
            break


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
    """Every file under tests/golden/lidar is accounted for: the fixtures by the digest of their arrays, the rest by name."""
    manifest = json.load(open(os.path.join(LIDAR_DIR, "MANIFEST.json")))
    assert sorted(manifest) == sorted(FIXTURES)
    files = sorted(f for f in os.listdir(LIDAR_DIR) if not f.startswith("__"))
    assert files == sorted([n + ".npz" for n in FIXTURES] + ["MANIFEST.json", "README.md", "make_golden_lidar.py"])
    for name in FIXTURES:
        path = os.path.join(LIDAR_DIR, name + ".npz")
        assert os.path.getsize(path) <= 290 * 1024, name
        with np.load(path) as z:
            assert _digest(z) == manifest[name], name


def test_fixtures_cover_what_they_are_for():
    z = {n: LidarGolden(n) for n in FIXTURES}
    assert (z["lidar_fast"].N, z["lidar_fast"].config["lanes_count"], z["lidar_fast"].z["obs"].shape[-2]) == (51, 4, 16)
    assert z["lidar_v0"].T == 15 and not z["lidar_v0"].fast
    raw = z["lidar_cells64_raw"]
    assert raw.z["obs"].shape[-2:] == (64, 2) and raw.z["obs"].max() == np.float32(35.0) and raw.z["obs"][..., 0].min() > 1.0
    ma = z["lidar_ma2"]
    a0, a1 = ma.hwy_config().agent_index[:2]
    gap = np.hypot(ma.z["init_x"][:, a0] - ma.z["init_x"][:, a1], ma.z["init_y"][:, a0] - ma.z["init_y"][:, a1])
    assert ma.A == 2 and (gap < 120.0).all()  # (within maximum_range of each other)
    assert z["lidar_n100"].N == 101
    assert z["lidar_linear"].config["other_vehicles_type"] == LINEAR and z["lidar_linear"].z["init_behavior"].any()
    d = z["lidar_direct"]
    assert d.config["action"]["type"] == "DiscreteAction" and np.abs(d.z["step_heading"][:, :, 0]).max() > 0.3
    cr = z["lidar_crash"]
    # crashed vehicles next to the observer: rectangles that touch or overlap it (a ray distance of a metre, the half width).  The
    # reference pushes colliding rectangles apart every frame (Vehicle.handle_collisions), so centres never come within WIDTH / 2
    # of each other in a run -- 160 more seeds of this configuration were searched, smallest distance 1.017 m -- and the NEGATIVE
    # centre distance is lidar_crafted's road 13
    crashed_ego = cr.z["step_crashed"][:, :, 0] != 0
    assert crashed_ego.any() and (cr.z["obs"][..., 0][crashed_ego] * 40.0).min() < 1.5
    assert (z["lidar_crafted"].z["obs0"][13, 0, :, 0] < 0).any()
    for g in z.values():
        assert g.z["obs0"].dtype == np.float32 and np.isfinite(g.z["obs0"]).all()


@pytest.mark.reference
@pytest.mark.skipif(not ref_stub.reference_available(), reason="needs the reference package")
@pytest.mark.parametrize("name", FIXTURES)
def test_env0_regenerates_bit_for_bit(name):
    mgl = sys.modules.get("make_golden_lidar")
    if mgl is None:
        spec = importlib.util.spec_from_file_location("make_golden_lidar", os.path.join(LIDAR_DIR, "make_golden_lidar.py"))
        mgl = importlib.util.module_from_spec(spec)
        sys.modules["make_golden_lidar"] = mgl
        spec.loader.exec_module(mgl)
    got = mgl.generate(name, only_envs={0})
    with np.load(os.path.join(LIDAR_DIR, name + ".npz")) as z:
        for k in z.files:
            a = z[k]
            if k.startswith(("init_", "obs0")):
                np.testing.assert_array_equal(got[k][0], a[0], err_msg=k)
            elif k.startswith("step_") or k in ("obs", "reward", "terminated", "truncated"):
                np.testing.assert_array_equal(got[k][:, 0], a[:, 0], err_msg=k)
            elif k not in ("meta", "seeds"):
                np.testing.assert_array_equal(got[k], a, err_msg=k)
