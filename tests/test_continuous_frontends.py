"""The front ends of continuous control: ``BatchedHighwayEnv.step_continuous``, the single-environment drop-ins and
``HighwayVectorEnv(..., continuous=True)`` -- spaces, accepted shapes, the float64 rounding rule, every error the interface names,
and the torch path (aliasing device tensors, every autoreset mode, ``rollout``) against the numpy path, bit for bit."""
import numpy as np
import pytest

from highwayenv_amd import _abi, envs, vector
from tests.continuous_util import BACKENDS, env_class, restate

F32 = np.float32
ACT = {"type": "DiscreteAction", "acceleration_range": [-3.3, 2.1], "steering_range": [-0.07, 0.05]}
CFG = {"vehicles_count": 20, "lanes_count": 3, "duration": 3, "action": ACT}
MA = {"vehicles_count": 20, "lanes_count": 3, "duration": 3, "controlled_vehicles": 2,
      "observation": {"type": "MultiAgentObservation", "observation_config": {"type": "Kinematics"}},
      "action": {"type": "MultiAgentAction", "action_config": ACT}}


def _venv(backend, cfg=CFG, E=4, base=envs.BatchedHighwayEnvFast, **kw):
    return vector.HighwayVectorEnv(env_class(backend, base), num_envs=E, config=cfg, **kw)


def test_the_config_type_stays_rejected_and_the_discrete_dict_names_the_continuous_one():
    with pytest.raises(NotImplementedError):
        _abi.make_config(dict(_abi.highway_default_config(), action={"type": "ContinuousAction"}), 2)
    p = _abi.continuous_params(ACT)
    assert (list(p.acceleration_range), list(p.steering_range), p.longitudinal, p.lateral, p.size) == ([-3.3, 2.1], [-0.07, 0.05], 1, 1, 2)
    d = _abi.continuous_params({"type": "DiscreteAction", "lateral": False})
    assert (list(d.acceleration_range), list(d.steering_range), d.size) == ([-5.0, 5.0], [-np.pi / 4, np.pi / 4], 1)
    with pytest.raises(NotImplementedError):
        _abi.continuous_params(dict(ACT, clip=False))
    with pytest.raises(ValueError):
        _abi.continuous_params(dict(ACT, longitudinal=False, lateral=False))
    with pytest.raises(ValueError):
        _abi.continuous_params(dict(ACT, steering_range=[-1.2, 1.2]))


def test_errors_that_need_no_engine():
    """Raised before any engine exists (no GPU needed): a DiscreteMetaAction ego, ``clip: False``, and the vector env's ValueError."""
    meta = envs.BatchedHighwayEnvFast({"vehicles_count": 5}, num_envs=2)
    with pytest.raises(NotImplementedError, match="DiscreteAction"):
        meta.step_continuous(np.zeros(2, F32))
    unclipped = envs.BatchedHighwayEnvFast(dict(CFG, action=dict(ACT, clip=False)), num_envs=2)
    with pytest.raises(NotImplementedError, match="clip"):
        unclipped.step_continuous(np.zeros(2, F32))
    for env_id in ("highway-fast-v0", "merge-v0", "intersection-v0"):  # DiscreteMetaAction defaults
        with pytest.raises(ValueError, match="DiscreteAction"):
            vector.HighwayVectorEnv(env_id, num_envs=2, continuous=True)


@pytest.mark.parametrize("backend", BACKENDS)
def test_spaces_shapes_and_the_float64_rule(backend):
    E = 4
    venv = _venv(backend, E=E, continuous=True)
    sp = venv.single_action_space
    assert tuple(sp.shape) == (2,) and np.dtype(sp.dtype) == np.float32 and float(np.min(sp.low)) == -1.0 and float(np.max(sp.high)) == 1.0
    assert tuple(venv.action_space.shape) == (E, 2)
    assert tuple(_venv(backend, dict(CFG, action=dict(ACT, lateral=False)), continuous=True).single_action_space.shape) == (1,)
    assert tuple(_venv(backend, MA, continuous=True).single_action_space.shape) == (2,)  # several agents: as for Discrete
    assert _venv(backend, E=E).single_action_space.n == 9                                 # (not continuous: unchanged)
    env = venv.env
    venv.reset(seed=3)
    p = env.continuous_params()
    # (size,), (E, size) and (E, A, size) of the same values are the same step; info["action"] echoes the float32 array
    a64 = np.random.default_rng(1).uniform(-1.3, 1.3, size=(E, 2))  # float64: rounded to float32 FIRST
    outs = []
    for shape in ((E, 2), (E, 1, 2)):
        venv.reset(seed=3)
        out = env.step_continuous(a64.reshape(shape))
        outs.append(out)
        assert out[4]["action"].dtype == np.float32 and out[4]["action"].shape == (E, 2)
        np.testing.assert_array_equal(out[4]["action"], a64.astype(F32))
        accel, steer = env._engine.get_controls()
        want = restate(p, a64.astype(F32))
        alive = ~(out[2] | out[3]) & ~out[4]["crashed"]
        np.testing.assert_array_equal(accel[alive, 0], want[0][alive])  # the float32 value's mapping, not the float64 one's
        np.testing.assert_array_equal(steer[alive, 0], want[1][alive])
    for x, y in zip(outs[0][:4], outs[1][:4]):
        np.testing.assert_array_equal(x, y)
    venv.reset(seed=3)
    one = env.step_continuous(a64[0])          # (size,): every environment
    venv.reset(seed=3)
    same = env.step_continuous(np.broadcast_to(a64[0].astype(F32), (E, 2)))
    for x, y in zip(one[:4], same[:4]):
        np.testing.assert_array_equal(x, y)
    for bad in (np.zeros(3), np.zeros((E, 3)), np.zeros((E + 1, 2)), np.zeros((E, 2, 2))):
        with pytest.raises(ValueError):
            env.step_continuous(bad)
    nan = np.zeros((E, 2), F32)
    nan[1, 0] = np.nan
    with pytest.raises(ValueError):
        env.step_continuous(nan)
    venv.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_scope_errors_of_a_direct_ego_are_unchanged(backend):
    venv = _venv(backend, continuous=True)
    venv.reset(seed=0)
    env = venv.env
    for call in (lambda: env.plan_lookahead(1), lambda: env.plan_opd(masked=True), env.get_available_actions, env.to_finite_mdp):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises((ValueError, IndexError, TypeError, NotImplementedError)):  # float sequences: the follow-up, not served
        env.score_sequences(np.full((2, 2), 0.5))
    venv.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_two_agents_and_the_single_environment_drop_in(backend):
    E = 3
    venv = _venv(backend, MA, E=E, continuous=True)
    venv.reset(seed=5)
    a = np.random.default_rng(2).uniform(-1, 1, size=(E, 2, 2)).astype(F32)
    obs, reward, term, trunc, info = venv.env.step_continuous(a)
    assert obs.shape[:2] == (E, 2) and info["action"].shape == (E, 2, 2) and info["agents_rewards"].shape == (E, 2)
    accel, steer = venv.env._engine.get_controls()
    want = restate(venv.env.continuous_params(), a)
    ok = ~info["agents_crashed"]
    np.testing.assert_array_equal(accel[ok], want[0][ok])
    np.testing.assert_array_equal(steer[ok], want[1][ok])
    venv.close()
    single = env_class(backend, envs.HighwayEnvFast)(CFG)
    single.reset(seed=1)
    obs, reward, term, trunc, info = single.step_continuous(np.array([0.3, -0.2]))
    assert obs.shape == (5, 5) and isinstance(reward, float) and isinstance(term, bool) and info["action"].dtype == np.float32
    assert single._engine.get_controls()[0][0, 0] == restate(single.continuous_params(), np.array([[0.3, -0.2]], F32))[0][0]
    single.close()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("mode", ["NextStep", "SameStep", "Disabled"])
def test_vector_env_numpy_modes_follow_the_discrete_run_on_grid_points(backend, mode):
    """Every autoreset mode of the numpy path: the continuous vector env on grid points is the DiscreteAction one on their ids."""
    E = 4
    cont, disc = _venv(backend, E=E, continuous=True, autoreset_mode=mode), _venv(backend, E=E, autoreset_mode=mode)
    o0, o1 = cont.reset(seed=11)[0], disc.reset(seed=11)[0]
    np.testing.assert_array_equal(o0, o1)
    axis = np.linspace(-1, 1, 3, dtype=F32)
    rng = np.random.default_rng(9)
    for t in range(6):
        ids = rng.integers(0, 9, size=E)
        cont.step_async(np.stack([axis[ids // 3], axis[ids % 3]], -1))
        a, b = cont.step_wait(), disc.step(ids)
        for j in range(4):
            np.testing.assert_array_equal(a[j], b[j], err_msg=f"{mode} step {t} output {j}")
        assert set(a[4]) == set(b[4])
        if "final_obs" in a[4]:
            for e in np.flatnonzero(a[4]["_final_obs"]):
                np.testing.assert_array_equal(a[4]["final_obs"][e], b[4]["final_obs"][e])
    cont.close()
    disc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["NextStep", "SameStep", "Disabled"])
@pytest.mark.parametrize("cfg", [CFG, MA], ids=["one-agent", "two-agents"])
def test_torch_path_aliases_its_buffers_and_equals_the_numpy_path(mode, cfg):
    """``output="torch"``: a contiguous float32 device tensor goes to the kernel as it is, the outputs alias the engine's buffers
    (the same storage every step), and -- NextStep and Disabled -- every output equals the numpy path's bit for bit.  SameStep runs
    the device sequence (hwy_step_same_step_continuous_device): the dense ``final_obs`` rows under the mask are the DiscreteAction
    torch env's on the grid ids, like everything else it returns."""
    import torch
    E, A = 64, cfg.get("controlled_vehicles", 1)
    tv = vector.HighwayVectorEnv("highway-fast-v0", num_envs=E, config=cfg, continuous=True, output="torch", autoreset_mode=mode)
    if mode == "SameStep":  # (the numpy SameStep re-spawns from another seed stream: the torch DiscreteAction env is the yardstick)
        other = vector.HighwayVectorEnv("highway-fast-v0", num_envs=E, config=cfg, output="torch", autoreset_mode=mode)
    else:
        other = vector.HighwayVectorEnv("highway-fast-v0", num_envs=E, config=cfg, continuous=True, autoreset_mode=mode)
    tv.reset(seed=21)
    other.reset(seed=21)
    axis = np.linspace(-1, 1, 3, dtype=F32)
    rng = np.random.default_rng(4)
    ptrs, ended = None, 0
    for t in range(7):
        ids = rng.integers(0, 9, size=(E, A))
        pts = np.stack([axis[ids // 3], axis[ids % 3]], -1).reshape((E, 2) if A == 1 else (E, A, 2))
        act = torch.from_numpy(pts).cuda()
        out = tv.step(act)
        assert all(x.is_cuda for x in out[:4]) and out[0].dtype == torch.float32 and out[1].dtype == torch.float64
        now = tuple(x.data_ptr() for x in out[:4])
        assert ptrs is None or now == ptrs  # the same buffers every step: views of what the kernel writes
        ptrs = now
        if mode == "SameStep":
            ref = other.step(torch.from_numpy(ids.reshape(E) if A == 1 else ids).to("cuda", torch.int32))
            host = lambda x: x.cpu().numpy()  # noqa: E731
            m = host(out[4]["_final_obs"])
            np.testing.assert_array_equal(m, host(ref[4]["_final_obs"]))
            np.testing.assert_array_equal(host(out[4]["final_obs"])[m], host(ref[4]["final_obs"])[m])
            np.testing.assert_array_equal(host(out[4]["final_info"]["speed"])[m], host(ref[4]["final_info"]["speed"])[m])
            ended += int(m.sum())
            ref = tuple(host(x) for x in ref[:4]) + ({k: host(ref[4][k]) for k in ("speed", "crashed")},)
        else:
            ref = other.step(pts)
        for j in range(4):
            np.testing.assert_array_equal(out[j].cpu().numpy(), ref[j], err_msg=f"{mode} step {t} output {j}")
        for k in ("speed", "crashed"):
            np.testing.assert_array_equal(out[4][k].cpu().numpy(), ref[4][k], err_msg=f"{mode} step {t} info {k}")
    assert mode != "SameStep" or ended >= E
    tv.close()
    other.close()


@pytest.mark.gpu
def test_torch_rollout_is_k_steps():
    import torch
    E, K = 64, 4
    a, b = (vector.HighwayVectorEnv("highway-fast-v0", num_envs=E, config=CFG, continuous=True, output="torch") for _ in range(2))
    a.reset(seed=8)
    b.reset(seed=8)
    acts = torch.from_numpy(np.random.default_rng(6).uniform(-1.3, 1.3, size=(K, E, 2)).astype(F32)).cuda()
    ro = a.rollout(acts)
    for k in range(K):
        out = b.step(acts[k])
        for j in range(4):
            assert torch.equal(ro[j][k], out[j]), (k, j)
    assert (ro[2] | ro[3])[:-1].any()  # duration 3: episodes end inside, the next step re-spawns them
    a.close()
    b.close()
