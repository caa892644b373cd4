"""The action mask on the MI355X: the HIP kernel equals the CPU emulation of the same source on the engine's own states over
auto-resetting steps (every scenario family, the one-wavefront and the workgroup step kernels' engines), the device-pointer form
equals the host-pointer form, ``HighwayVectorEnv(output="torch", action_masks=True)`` hands out the device tensor the kernel wrote,
and ``plan_lookahead(masked=True)`` masks the first action only."""
import numpy as np
import pytest

from highwayenv_amd import _abi, envs
from highwayenv_amd.vector import HighwayVectorEnv

pytestmark = pytest.mark.gpu

MA = {"observation": {"type": "MultiAgentObservation", "observation_config": {"type": "Kinematics"}},
      "action": {"type": "MultiAgentAction", "action_config": {"type": "DiscreteMetaAction"}}}
# (environment id, config, environments): N = 20 and N = 130 (the workgroup step kernel's engine) on the highway, merge-generic
# with 4 agents, the intersection with 15 slots
SHAPES = [("highway-fast-v0", {"vehicles_count": 19}, 5), ("highway-fast-v0", {"vehicles_count": 129, "lanes_count": 4}, 3),
          ("merge-generic-v0", dict(MA, controlled_vehicles=4, lanes_count=4, vehicles_count=20), 4),
          ("intersection-v0", {"initial_vehicle_count": 5, "spawn_probability": 0.6}, 6)]


def _hip_vs_emulator(env_id, config, E, steps=10):
    from tests.emu import emu
    cls = envs.batched_class(env_id)
    env = cls(dict(config), num_envs=E, spawn_mode="device", autoreset=True)
    env.reset(seed=11)
    cfg, rng = env._hcfg, np.random.default_rng(3)
    n_ids, A = _abi.num_actions(cfg), cfg.num_agents
    seen = np.zeros(n_ids, int)
    for t in range(steps + 1):
        got = env._engine.action_mask()
        want = emu.action_mask(cfg, env._engine.get_state())
        np.testing.assert_array_equal(got, want, err_msg=f"{env_id} step {t}")
        seen += got.reshape(-1, n_ids).sum(axis=0)
        env.step(rng.integers(0, n_ids, size=(E, A)))
    assert seen[1] == (steps + 1) * E * A and (seen > 0).all() and (seen[[0, 2]] < seen[1]).all()
    env.close()
    return cfg


@pytest.mark.parametrize("env_id,config,E", SHAPES, ids=["n20", "n130", "merge_generic_ma4", "intersection15"])
def test_hip_equals_emulator_on_the_engines_own_states(env_id, config, E):
    cfg = _hip_vs_emulator(env_id, config, E)
    if env_id == "intersection-v0":
        assert cfg.num_vehicles >= 15


def test_device_pointer_form_equals_host_pointer_form():
    import torch
    env = envs.BatchedHighwayEnvFast({"vehicles_count": 12}, num_envs=300, spawn_mode="device")   # more than one workgroup
    env.reset(seed=2)
    env.step(np.random.default_rng(0).integers(0, 5, 300))
    host = env._engine.action_mask()
    out = torch.full((300, 1, 5), 7, dtype=torch.uint8, device="cuda")
    env._engine.action_mask_device(out.data_ptr())
    env._engine.sync()
    np.testing.assert_array_equal(out.cpu().numpy().astype(bool), host)
    assert int(out.max()) == 1
    env.close()


@pytest.mark.parametrize("mode", ["NextStep", "Disabled"])
def test_torch_vector_env_mask_is_the_device_tensor(mode):
    """info["action_mask"] of output="torch" is a bool device tensor that equals the numpy front end's over 5 steps; with
    action_masks=False the outputs are bit-identical to a run without the argument.  The torch front end runs in the NextStep and
    Disabled autoreset modes only (it refuses SameStep, which merges a masked reset on the host: INTEGRATION.md), so these two modes
    stand for "NextStep and SameStep" here, and SameStep is held with numpy outputs in test_same_step_numpy_vector_env_mask."""
    import torch
    cfg = {"vehicles_count": 10, "duration": 3}
    kw = dict(num_envs=6, config=cfg, autoreset_mode=mode)
    tv = HighwayVectorEnv("highway-fast-v0", output="torch", action_masks=True, **kw)
    nv = HighwayVectorEnv("highway-fast-v0", action_masks=True, **kw)
    off = HighwayVectorEnv("highway-fast-v0", output="torch", action_masks=False, **kw)
    plain = HighwayVectorEnv("highway-fast-v0", output="torch", **kw)
    _, ti = tv.reset(seed=9)
    _, ni = nv.reset(seed=9)
    _, oi = off.reset(seed=9)
    plain.reset(seed=9)
    assert "action_mask" not in oi
    m = ti["action_mask"]
    assert isinstance(m, torch.Tensor) and m.is_cuda and m.dtype == torch.bool and tuple(m.shape) == (6, 5)
    assert m.data_ptr() == tv._dev["action_mask"].data_ptr()   # the buffer the kernel wrote: no copy
    np.testing.assert_array_equal(m.cpu().numpy(), ni["action_mask"])
    rng = np.random.default_rng(4)
    for t in range(5):
        a = rng.integers(0, 5, 6)
        to, tr, tt, tu, ti = tv.step(a)
        no, nr, nt, nu, ni = nv.step(a)
        np.testing.assert_array_equal(ti["action_mask"].cpu().numpy(), ni["action_mask"], err_msg=f"step {t}")
        np.testing.assert_array_equal(to.cpu().numpy(), no)
        oo, orw, ot, ou, oi = off.step(a)
        po, prw, pt, pu, pi = plain.step(a)
        assert "action_mask" not in oi and set(oi) == set(pi)
        for x, y in ((oo, po), (orw, prw), (ot, pt), (ou, pu), (oi["speed"], pi["speed"]), (oi["crashed"], pi["crashed"])):
            assert torch.equal(x, y)
    for v in (tv, nv, off, plain):
        v.close()


def test_same_step_numpy_vector_env_mask():
    cfg = {"vehicles_count": 10, "duration": 2}
    venv = HighwayVectorEnv("highway-fast-v0", num_envs=4, config=cfg, autoreset_mode="SameStep", action_masks=True)
    venv.reset(seed=1)
    ended = 0
    for t in range(5):
        _, _, term, trunc, info = venv.step(np.full(4, 1))
        np.testing.assert_array_equal(info["action_mask"], venv.env.get_available_actions())
        for e in np.flatnonzero(term | trunc):
            assert info["final_info"][e]["action_mask"].shape == (5,)
            ended += 1
    assert ended >= 4
    venv.close()


@pytest.mark.parametrize("output", ["numpy", "torch"])
def test_masked_lookahead_masks_the_first_action_only(output):
    venv = HighwayVectorEnv("highway-fast-v0", num_envs=8, config={"vehicles_count": 15, "lanes_count": 3}, output=output,
                            autoreset_mode="Disabled")
    venv.reset(seed=3)
    venv.step(np.array([0, 0, 2, 2, 3, 3, 4, 4]))   # to the edges of the road and the ends of the speed ladder
    venv.step(np.array([0, 0, 2, 2, 3, 3, 4, 4]))
    a0, q0 = venv.plan_lookahead(2, return_q=True)
    a1, q1 = venv.plan_lookahead(2, return_q=True, masked=True)
    to_np = (lambda x: x.cpu().numpy()) if output == "torch" else np.asarray
    a0, q0, a1, q1 = to_np(a0), to_np(q0), to_np(a1), to_np(q1)
    mask = venv.env.get_available_actions()
    assert (~mask).any() and mask[:, 1].all()
    assert np.all(np.isneginf(q1[~mask])) and np.array_equal(q1[mask], q0[mask])   # -inf exactly on the unavailable first actions
    np.testing.assert_array_equal(a1, np.where(mask, q0, -np.inf).argmax(axis=1))
    assert mask[np.arange(8), a1].all()
    venv.close()
