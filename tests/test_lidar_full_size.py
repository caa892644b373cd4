"""LidarObservation at the headline shape on the MI355X: 4096 environments x 51 vehicles (highway-fast-v0, 50 vehicles, 4 lanes),
16 cells, device spawn, 30 policy steps with auto-reset.  64 environments spread over the batch are followed step by step by the
CPU emulation of the same kernel source from the engine's own states; every environment's observation is checked for the
properties any lidar observation has."""
import numpy as np
import pytest

from highwayenv_amd import _abi

E, STEPS, CELLS = 4096, 30, 16


@pytest.mark.gpu
def test_headline_shape_hip_equals_emulator_and_properties():
    from highwayenv_amd.engine import Engine
    from tests.emu import emu
    cfg_d = _abi.highway_fast_default_config()
    cfg_d.update({"vehicles_count": 50, "lanes_count": 4, "observation": {"type": "LidarObservation", "cells": CELLS}})
    cfg = _abi.make_config(cfg_d, E, fast=True)
    assert (cfg.num_envs, cfg.num_vehicles) == (4096, 51)
    eng = Engine(cfg)
    watch = np.arange(0, E, E // 64)
    assert len(watch) == 64
    sub = _abi.make_config(cfg_d, len(watch), fast=True)

    def check(obs, st, what):
        assert obs.shape == (E, 1, CELLS, 2) and obs.dtype == np.float32
        assert np.isfinite(obs).all(), what
        dist, vel = obs[..., 0], obs[..., 1]
        assert dist.min() >= -1.0 and dist.max() <= 1.0, (what, float(dist.min()), float(dist.max()))
        untouched = dist == 1.0  # (a traced distance is below maximum_range - WIDTH / 2 rounded, never exactly the range)
        assert (vel[untouched] == 1.0).all(), what
        assert untouched.any() and (~untouched).any(), what
        # |relative radial speed| <= |v_obstacle| + |v_observer| <= 2 * MAX_SPEED = 80 m/s
        assert np.abs(vel[~untouched]).max() <= 80.0 / 60.0, what
        want = emu.trace(sub, {k: np.ascontiguousarray(v[watch]) for k, v in st.items()})
        bad = np.abs(obs[watch].astype(np.float64) - want) > 1e-6
        assert not bad.any(), f"{what}: {int(bad.any(-1).sum())} of {want[..., 0].size} watched cells differ from the emulation"

    obs = eng.reset(base_seed=2024, ego_spacing=cfg_d["ego_spacing"], vehicles_density=cfg_d["vehicles_density"])
    check(obs, eng.get_state(), "reset")
    np.testing.assert_array_equal(eng.observe().view(np.uint32), obs.view(np.uint32))
    eng.set_autoreset(True, base_seed=99, ego_spacing=cfg_d["ego_spacing"], vehicles_density=cfg_d["vehicles_density"])
    rng = np.random.default_rng(5)
    ended = 0
    for t in range(STEPS):
        obs, reward, term, trunc, info = eng.step(rng.integers(0, 5, size=(E, 1)).astype(np.int32))
        check(obs, eng.get_state(), f"step {t}")
        ended += int((term | trunc).sum())
    assert eng.counters()["nonfinite_stores"] == 0
    assert ended > 0  # (auto-reset steps were among the ones checked)
    eng.close()


@pytest.mark.gpu
def test_vector_env_torch_output_is_the_lidar_device_tensor():
    """HighwayVectorEnv(output="torch") with a LidarObservation: step and rollout return device tensors [E, cells, 2] that hold what
    the numpy path of an identically seeded environment returns."""
    import torch

    from highwayenv_amd import vector
    cfg = {"vehicles_count": 20, "observation": {"type": "LidarObservation", "cells": 12, "maximum_range": 50}}
    t = vector.HighwayVectorEnv("highway-fast-v0", num_envs=16, config=cfg, output="torch")
    n = vector.HighwayVectorEnv("highway-fast-v0", num_envs=16, config=cfg)
    o_t, _ = t.reset(seed=3)
    o_n, _ = n.reset(seed=3)
    assert isinstance(o_t, torch.Tensor) and o_t.is_cuda and tuple(o_t.shape) == (16, 12, 2) and o_t.dtype == torch.float32
    assert t.single_observation_space.shape == (12, 2)
    np.testing.assert_array_equal(o_t.cpu().numpy().view(np.uint32), o_n.view(np.uint32))
    rng = np.random.default_rng(0)
    for _ in range(5):
        a = rng.integers(0, 5, size=16)
        o_t, r_t, te_t, tr_t, _ = t.step(a)
        o_n, r_n, te_n, tr_n, _ = n.step(a)
        assert o_t.is_cuda and tuple(o_t.shape) == (16, 12, 2)
        np.testing.assert_array_equal(o_t.cpu().numpy().view(np.uint32), np.asarray(o_n).view(np.uint32))
        np.testing.assert_array_equal(r_t.cpu().numpy(), r_n)
    acts = rng.integers(0, 5, size=(3, 16))
    ro = t.rollout(torch.as_tensor(acts))
    assert ro[0].is_cuda and tuple(ro[0].shape) == (3, 16, 12, 2)
    for k in range(3):
        o_n, *_ = n.step(acts[k])
        np.testing.assert_array_equal(ro[0][k].cpu().numpy().view(np.uint32), np.asarray(o_n).view(np.uint32))
    t.close()
    n.close()
