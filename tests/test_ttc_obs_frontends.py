"""The front ends of the TimeToCollision observation: ``BatchedHighwayEnv.ttc_observation`` / ``ttc_observation_space``, the
single-environment drop-ins and ``HighwayVectorEnv(..., ttc_observation=True | {"horizon": h})`` -- spaces, shapes, every error the
interface names, NumPy output on the CPU emulation and on the GPU, and the torch path (device tensors, no synchronisation in
``step``, NextStep and SameStep, ``rollout``) against the NumPy path, bit for bit."""
import numpy as np
import pytest

from highwayenv_amd import _abi, envs, vector
from tests.backends import BACKENDS

CFG = {"vehicles_count": 20, "lanes_count": 3, "duration": 3, "vehicles_density": 2.0}
MA = dict(CFG, controlled_vehicles=2, observation={"type": "MultiAgentObservation", "observation_config": {"type": "Kinematics"}},
          action={"type": "MultiAgentAction", "action_config": {"type": "DiscreteMetaAction"}})
DIRECT = dict(CFG, action={"type": "DiscreteAction"})
FASTER = 3


def env_class(backend, base):
    if backend != "emu":
        return base
    from tests.emu.emu_ttc_obs import TtcObsEmuEngine
    return type("Emu" + base.__name__, (base,), {"_engine_factory": staticmethod(lambda cfg, device, stream: TtcObsEmuEngine(cfg))})


def _venv(backend, cfg=CFG, E=4, base=envs.BatchedHighwayEnvFast, **kw):
    return vector.HighwayVectorEnv(env_class(backend, base), num_envs=E, config=cfg, **kw)


def _box(space, shape):
    assert tuple(space.shape) == shape and np.dtype(space.dtype) == np.float32
    assert float(np.min(space.low)) == 0.0 and float(np.max(space.high)) == 1.0


def test_the_config_type_stays_rejected():
    for obs in ({"type": "TimeToCollision"}, {"type": "TimeToCollision", "horizon": 5},
                {"type": "MultiAgentObservation", "observation_config": {"type": "TimeToCollision"}}):
        with pytest.raises(NotImplementedError):
            _abi.make_config(dict(_abi.highway_default_config(), observation=obs), 2)
        # ... while the same config without the type serves the observation through its own door
        A = 2 if obs["type"] == "MultiAgentObservation" else 1
        env = envs.BatchedHighwayEnv(dict(MA, duration=40) if A == 2 else None, num_envs=2)
        space = env.ttc_observation_space(obs.get("horizon", 10))
        _box(space if A == 1 else space.spaces[1], (3, 3, obs.get("horizon", 10)))


def test_errors_that_need_no_engine():
    """Before reset(), off the highway, with a DiscreteAction ego: NotImplementedError; with continuous=True: ValueError."""
    env = envs.BatchedHighwayEnvFast(dict(CFG), num_envs=2)
    with pytest.raises(NotImplementedError, match="initialized"):
        env.ttc_observation()
    _box(env.ttc_observation_space(), (3, 3, 10))             # (the space needs the config only)
    _box(env.ttc_observation_space(horizon=5), (3, 3, 5))
    for bad in (envs.BatchedMergeEnv(num_envs=2), envs.BatchedIntersectionEnv(num_envs=2), envs.BatchedHighwayEnvFast(dict(DIRECT), num_envs=2)):
        for call in (bad.ttc_observation, bad.ttc_observation_space):
            with pytest.raises(NotImplementedError):
                call()
    with pytest.raises(ValueError):                           # 65 time steps
        env.ttc_observation_space(horizon=65)
    with pytest.raises(ValueError, match="not together"):
        vector.HighwayVectorEnv(envs.BatchedHighwayEnvFast, num_envs=2, config=DIRECT, continuous=True, ttc_observation=True)
    for env_id in ("merge-v0", "intersection-v0"):
        with pytest.raises(NotImplementedError):
            vector.HighwayVectorEnv(env_id, num_envs=2, ttc_observation=True)
    with pytest.raises(NotImplementedError):
        vector.HighwayVectorEnv(envs.BatchedHighwayEnvFast, num_envs=2, config=DIRECT, ttc_observation=True)


@pytest.mark.parametrize("backend", BACKENDS)
def test_batched_env_and_drop_ins(backend):
    E = 3
    env = env_class(backend, envs.BatchedHighwayEnvFast)(dict(CFG), num_envs=E)
    obs, _ = env.reset(seed=1)
    assert obs.shape == (E, 5, 5)                             # the configured observation is untouched
    w = env.ttc_observation()
    assert w.shape == (E, 3, 3, 10) and w.dtype == np.float32 and np.isin(w, (0.0, 0.5, 1.0)).all()
    assert env.ttc_observation(horizon=5).shape == (E, 3, 3, 5)
    np.testing.assert_array_equal(env.ttc_observation(horizon=5), w[..., :5])
    # the window of the device's own grid
    st, grid = env.get_state(), env.ttc_grid()
    from tests.ttc_obs_util import windows
    np.testing.assert_array_equal(w, windows(env._hcfg, st, grid)[:, 0].astype(np.float32))
    env.close()
    ma = env_class(backend, envs.BatchedHighwayEnvFast)(dict(MA), num_envs=E)
    ma.reset(seed=2)
    assert ma.ttc_observation().shape == (E, 2, 3, 3, 10)
    space = ma.ttc_observation_space()
    assert len(space.spaces) == 2
    _box(space.spaces[0], (3, 3, 10))
    ma.close()
    one = env_class(backend, envs.HighwayEnvFast)(dict(CFG))
    one.reset(seed=3)
    w1 = one.ttc_observation()
    assert w1.shape == (3, 3, 10) and w1.dtype == np.float32
    one.step(FASTER)
    assert one.ttc_observation(horizon=4).shape == (3, 3, 4)
    one.close()
    two = env_class(backend, envs.HighwayEnvFast)(dict(MA))
    two.reset(seed=4)
    pair = two.ttc_observation()
    assert isinstance(pair, tuple) and len(pair) == 2 and all(p.shape == (3, 3, 10) for p in pair)
    two.close()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("mode", ["NextStep", "SameStep", "Disabled"])
def test_vector_env_numpy_output(backend, mode):
    E = 4
    venv = _venv(backend, E=E, autoreset_mode=mode, ttc_observation={"horizon": 6})
    _box(venv.single_observation_space, (3, 3, 6))
    assert tuple(venv.observation_space.shape) == (E, 3, 3, 6)
    obs, info = venv.reset(seed=7)
    assert obs.shape == (E, 3, 3, 6) and obs.dtype == np.float32
    np.testing.assert_array_equal(obs, venv.env.ttc_observation(6))
    ended = 0
    for _ in range(5):
        obs, reward, term, trunc, infos = venv.step(np.full(E, FASTER))
        assert obs.shape == (E, 3, 3, 6) and obs.dtype == np.float32 and reward.shape == (E,)
        np.testing.assert_array_equal(obs, venv.env.ttc_observation(6))  # the window of the state the call leaves
        done = term | trunc
        if mode == "SameStep" and done.any():
            ended += int(done.sum())
            np.testing.assert_array_equal(infos["_final_obs"], done)
            for e in range(E):
                assert (infos["final_obs"][e] is None) == (not done[e])
                if done[e]:
                    assert infos["final_obs"][e].shape == (3, 3, 6) and infos["final_obs"][e].dtype == np.float32
    assert mode != "SameStep" or ended, "no episode ended"
    venv.close()
    _box(_venv(backend, E=E, autoreset_mode=mode, ttc_observation={}).single_observation_space, (3, 3, 10))  # {}: the default horizon
    assert tuple(_venv(backend, E=E, autoreset_mode=mode, ttc_observation=None).single_observation_space.shape) == (5, 5)
    ma = _venv(backend, MA, E=3, autoreset_mode=mode, ttc_observation=True)
    assert len(ma.single_observation_space.spaces) == 2
    assert ma.reset(seed=8)[0].shape == (3, 2, 3, 3, 10)
    assert ma.step(np.full((3, 2), FASTER))[0].shape == (3, 2, 3, 3, 10)
    ma.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["NextStep", "SameStep"])
@pytest.mark.parametrize("cfg", [CFG, MA], ids=["one", "ma2"])
def test_torch_output_against_numpy_output(mode, cfg, monkeypatch):
    """The same seeds through output="numpy" and output="torch": the same windows, rewards and flags at every step; on torch they
    are device tensors and ``step`` synchronises nothing."""
    import torch
    E, A = 4, int(cfg.get("controlled_vehicles", 1))
    host = _venv("hip", cfg, E=E, autoreset_mode=mode, ttc_observation=True)
    dev = _venv("hip", cfg, E=E, autoreset_mode=mode, ttc_observation=True, output="torch")
    shape = (E, 3, 3, 10) if A == 1 else (E, A, 3, 3, 10)
    h0, _ = host.reset(seed=11)
    d0, _ = dev.reset(seed=11)
    assert d0.is_cuda and tuple(d0.shape) == shape
    np.testing.assert_array_equal(d0.cpu().numpy(), h0)
    actions = torch.full((E, A), FASTER, dtype=torch.int32, device="cuda")
    ended = 0
    for k in range(6):
        want = host.step(np.full((E, A), FASTER))

        def no_sync(*a, **kw):
            raise AssertionError("step() synchronised")
        with monkeypatch.context() as m:
            m.setattr(torch.cuda, "synchronize", no_sync)
            m.setattr(torch.cuda.Stream, "synchronize", no_sync)
            m.setattr(type(dev.env._engine), "sync", no_sync)
            got = dev.step(actions)
        assert all(x.is_cuda for x in got[:4]) and tuple(got[0].shape) == shape
        done = want[2] | want[3]
        if mode == "SameStep" and ended:  # (the re-spawns of the two paths draw different seeds: compared until an episode has ended)
            continue
        np.testing.assert_array_equal(got[1].cpu().numpy(), want[1], err_msg=f"step {k}: reward")
        np.testing.assert_array_equal(got[2].cpu().numpy(), want[2], err_msg=f"step {k}: terminated")
        np.testing.assert_array_equal(got[3].cpu().numpy(), want[3], err_msg=f"step {k}: truncated")
        if mode == "SameStep":
            np.testing.assert_array_equal(got[4]["_final_obs"].cpu().numpy(), done)
            f = got[4]["final_obs"].cpu().numpy()
            for e in np.flatnonzero(done):
                np.testing.assert_array_equal(f[e], want[4]["final_obs"][e], err_msg=f"step {k}: final_obs of {e}")
            np.testing.assert_array_equal(got[0].cpu().numpy()[~done], want[0][~done], err_msg=f"step {k}: obs of the others")
            ended += int(done.sum())
        else:
            np.testing.assert_array_equal(got[0].cpu().numpy(), want[0], err_msg=f"step {k}: obs")
    assert mode != "SameStep" or ended, "no step that ended an episode was compared"
    host.close()
    dev.close()


@pytest.mark.gpu
def test_torch_rollout_equals_steps():
    import torch
    E, K = 4, 5
    a = _venv("hip", E=E, ttc_observation=True, output="torch")
    b = _venv("hip", E=E, ttc_observation=True, output="torch")
    a.reset(seed=5)
    b.reset(seed=5)
    acts = torch.full((K, E), FASTER, dtype=torch.int32, device="cuda")
    obs, rew, term, trunc = a.rollout(acts)
    assert tuple(obs.shape) == (K, E, 3, 3, 10) and obs.is_cuda
    for k in range(K):
        o, r, te, tr, _ = b.step(acts[k])
        np.testing.assert_array_equal(obs[k].cpu().numpy(), o.cpu().numpy(), err_msg=f"step {k}")
        np.testing.assert_array_equal(rew[k].cpu().numpy(), r.cpu().numpy())
        np.testing.assert_array_equal(term[k].cpu().numpy(), te.cpu().numpy())
        np.testing.assert_array_equal(trunc[k].cpu().numpy(), tr.cpu().numpy())
    assert (term | trunc)[:-1].any(), "no auto-reset inside the rollout"
    with pytest.raises(ValueError):
        _venv("hip", E=E, ttc_observation=True).rollout(acts)
    a.close()
    b.close()
