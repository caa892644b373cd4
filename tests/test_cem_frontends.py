"""plan_cem through the front ends: the single-environment drop-ins (a 1-D action that step_continuous takes), the vector env on
NumPy and, on the GPU with output="torch", as the device tensor the refit kernel wrote -- env.step(env.plan_cem()) under every
autoreset mode without leaving the device."""
import numpy as np
import pytest

from highwayenv_amd import envs
from highwayenv_amd.vector import HighwayVectorEnv
from tests import cem_util as cu

KW = dict(population=5, elites=2, iterations=2, horizon=3)


@pytest.mark.parametrize("backend", cu.BACKENDS)
@pytest.mark.parametrize("size", [2, 1])
def test_drop_in_returns_a_one_d_action(backend, size):
    cls = cu.env_class(backend, envs.HighwayEnvFast)
    env = cls(cu.small_config(size=size))
    env.reset(seed=3)
    action = env.plan_cem(seed=4, **KW)
    assert action.shape == (size,) and action.dtype == np.float32 and (np.abs(action) <= 1).all()
    again, det = env.plan_cem(seed=4, return_details=True, debug=True, **KW)
    cu.assert_bits_equal(action, again)
    assert det["best_sequence"].shape == (3, size) and det["mean"].shape == (3, size) and det["std"].shape == (3, size)
    assert np.ndim(det["best_return"]) == 0 and det["noise"].shape == (2, 5, 3, size) and det["samples"].shape == (2, 5, 3, size)
    cu.assert_bits_equal(det["best_sequence"][0], action)
    # warm start: the mean shifted by one step goes back in
    shifted = np.concatenate([det["mean"][1:], det["mean"][-1:]])
    warm = env.plan_cem(seed=5, init_mean=shifted, **KW)
    assert warm.shape == (size,)
    obs, reward, term, trunc, info = env.step_continuous(action)
    assert np.isfinite(reward) and info["action"].shape == (size,)
    env.close()


@pytest.mark.parametrize("backend", cu.BACKENDS)
def test_vector_env_numpy(backend):
    venv = HighwayVectorEnv(cu.env_class(backend), num_envs=3, config=cu.small_config(), continuous=True)
    venv.reset(seed=1)
    action, det = venv.plan_cem(seed=2, return_details=True, **KW)
    assert action.shape == (3, 2) and action.dtype == np.float32 and det["best_return"].shape == (3,)
    cu.assert_bits_equal(action, venv.env.plan_cem(seed=2, **KW))
    obs, reward, term, trunc, infos = venv.step(action)
    assert reward.shape == (3,)
    venv.close()
    ids = HighwayVectorEnv(cu.env_class(backend), num_envs=2, config=cu.small_config())
    with pytest.raises(ValueError, match="continuous=True"):
        ids.plan_cem()
    ids.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["NextStep", "SameStep", "Disabled"])
def test_vector_env_torch_plans_and_steps_on_the_device(mode):
    torch = pytest.importorskip("torch")
    venv = HighwayVectorEnv("highway-fast-v0", num_envs=3, config=cu.small_config(), continuous=True, output="torch", autoreset_mode=mode)
    venv.reset(seed=1)
    action, det = venv.plan_cem(seed=2, return_details=True, **KW)
    assert isinstance(action, torch.Tensor) and action.is_cuda and action.dtype == torch.float32 and tuple(action.shape) == (3, 2)
    assert action.data_ptr() == venv._dev[("cem", 3)]["action"].data_ptr()   # the tensor the kernel wrote, not a copy
    # the same search through the host door of an equal environment
    ref = HighwayVectorEnv("highway-fast-v0", num_envs=3, config=cu.small_config(), continuous=True, autoreset_mode=mode)
    ref.reset(seed=1)
    want, wdet = ref.plan_cem(seed=2, return_details=True, **KW)
    cu.assert_bits_equal(action.cpu().numpy(), want, "action")
    for k in ("best_return", "best_sequence", "mean", "std"):
        cu.assert_bits_equal(det[k].cpu().numpy(), wdet[k], k)
    for _ in range(3):   # plan -> step, nothing visits the host
        obs, reward, term, trunc, infos = venv.step(venv.plan_cem(**KW))
    assert obs.is_cuda and torch.isfinite(reward).all()
    # the default seed on the device path: this front steps the engine without touching the env's step count, and still no two
    # decisions share noise -- two calls around a torch step, and two calls with no step between them
    _, n1 = venv.plan_cem(return_details=True, debug=True, **KW)
    n1 = {k: v.clone() for k, v in n1.items()}
    venv.step(torch.zeros((3, 2), dtype=torch.float32, device=action.device))
    _, n2 = venv.plan_cem(return_details=True, debug=True, **KW)
    _, n3 = venv.plan_cem(return_details=True, debug=True, **KW)
    for a, b in ((n1, n2), (n2, n3), (n1, n3)):
        assert (a["noise"][:, :, 1:] != b["noise"][:, :, 1:]).all() and (a["noise"][:, :, 0] == 0).all()
    assert tuple(n2["elites"].shape) == (2, 3, 2) and n2["elites"].dtype == torch.int32 and (n2["elites"][..., 0] < n2["elites"][..., 1]).all()
    # a warm start from a device tensor
    warm = venv.plan_cem(seed=3, init_mean=torch.roll(det["mean"], -1, dims=1), **KW)
    assert torch.isfinite(warm).all() and (warm.abs() <= 1).all()
    venv.close(), ref.close()
