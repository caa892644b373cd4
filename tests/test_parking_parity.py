"""The parking kernels (csrc/hwy_park.h) on the GPU against the unmodified reference's ParkingEnv (tests/golden/parking): every
fixture driven from its recorded initial state with its recorded actions, K steps in one launch against K launches, batches whose
neighbouring threads run different fixtures, the device reset against the rule on the suite's Python Philox, the goal reward."""
import glob
import json
import os

import numpy as np
import pytest

from highwayenv_amd import parking
from tests import spawn_util

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parking")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")) if "reset_rule" not in p)
# one kernel configuration (walls, 3 frames, duration 20): these run side by side in one batch
DEFAULT_GROUP = ["free_0", "wall_long", "parked_10", "success_in", "parked_26", "wall_short", "parked_10_free", "success_out", "free_1"]
BATCH_STEPS = 30
pytestmark = pytest.mark.gpu


def load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def initial_state(fixtures):
    st = parking.alloc_state(len(fixtures))
    for e, z in enumerate(fixtures):
        st["x"][e], st["y"][e], st["heading"][e], st["speed"][e] = z["init_ego"]
        st["goal"][e] = z["goal"]
        st["order"][e, :len(z["order"])] = z["order"]
        st["occupied"][e] = sum(1 << int(k) for k in z["order"])
    return st


def engine_for(z, num_envs, **kw):
    cfg = parking.parking_default_config()
    cfg.update(json.loads(str(z["config_json"])))
    return parking.ParkEngine(parking.make_park_config(cfg, num_envs, **kw))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("name", FIXTURES)
def test_teacher_forced_fixture(name):
    z = load(name)
    eng = engine_for(z, 1)
    eng.set_state(initial_state([z]))
    n = len(z["order"])
    for t in range(len(z["actions"])):
        obs, reward, flags = eng.advance(z["actions"][t].reshape(1, 1, 2))
        st = eng.get_state()
        ego = np.array([st[k][0] for k in parking.EGO_FIELDS[:8]])
        np.testing.assert_allclose(ego, z["ego"][t], rtol=0, atol=1e-9, err_msg=f"step {t}")
        assert np.array_equal(bits(ego[3:6]), bits(z["ego"][t, 3:6])), (t, ego[3:6], z["ego"][t, 3:6])  # speed, stored controls
        f = int(st["flags"][0])
        assert bool(f & parking.F_CRASHED) == z["ego_crashed"][t] and bool(f & parking.F_HAS_IMPACT) == z["ego_has_impact"][t], t
        struck = np.array([(int(st["struck"][0]) >> i) & 1 for i in range(n)], bool)
        sx, sy = parking.spot_position(z["order"])
        px, py = np.where(struck, st["parked_x"][0, :n], sx), np.where(struck, st["parked_y"][0, :n], sy)
        np.testing.assert_allclose(np.stack([px, py], 1), z["parked"][t, :, :2], rtol=0, atol=1e-9, err_msg=f"step {t}")
        np.testing.assert_array_equal(z["parked"][t, :, 2:], np.stack([parking.spot_heading(z["order"]), np.zeros(n)], 1))
        assert np.array_equal([(int(st["parked_crashed"][0]) >> i) & 1 for i in range(n)], z["parked_crashed"][t]), t
        np.testing.assert_allclose(obs[0], z["obs"][t], rtol=0, atol=1e-6, err_msg=f"step {t}")
        assert abs(reward[0] - z["reward"][t]) <= 1e-9, (t, reward[0], z["reward"][t])
        want = (z["terminated"][t] * parking.S_TERMINATED | z["truncated"][t] * parking.S_TRUNCATED
                | z["is_success"][t] * parking.S_SUCCESS | z["ego_crashed"][t] * parking.S_CRASHED)
        assert flags[0] == want, (t, flags[0], want)
    eng.close()


_singles = {}


def single_run(name):
    """One environment of fixture `name`, BATCH_STEPS steps (its actions, then zeros) in one launch: state, rewards, flags."""
    if name not in _singles:
        z = load(name)
        eng = engine_for(z, 1)
        eng.set_state(initial_state([z]))
        actions = np.zeros((BATCH_STEPS, 1, 2), np.float32)
        k = min(BATCH_STEPS, len(z["actions"]))
        actions[:k, 0] = z["actions"][:k]
        obs, _, _, sr, sf = eng.advance(actions, per_step=True)
        _singles[name] = (actions, obs, sr, sf, eng.get_state())
        eng.close()
    return _singles[name]


def test_k_steps_in_one_launch_are_k_launches():
    actions, obs, sr, sf, st = single_run("parked_10")
    eng = engine_for(load("parked_10"), 1)
    eng.set_state(initial_state([load("parked_10")]))
    for t in range(BATCH_STEPS):
        o1, r1, f1 = eng.advance(actions[t:t + 1])
        assert bits(r1)[0] == bits(sr[t])[0] and f1[0] == sf[t, 0], t
    assert np.array_equal(o1.view(np.uint32), obs.view(np.uint32))
    got = eng.get_state()
    assert all(np.array_equal(got[k], st[k]) for k in st)
    assert (sf[:, 0] & parking.S_CRASHED).any() and got["struck"][0] != 0  # the run covers a struck vehicle
    eng.close()


@pytest.mark.parametrize("E", [1, 64, 65, 257])
def test_batch_neighbours_run_different_fixtures(E):
    names = [DEFAULT_GROUP[e % len(DEFAULT_GROUP)] for e in range(E)]
    eng = engine_for(load(names[0]), E)
    eng.set_state(initial_state([load(n) for n in names]))
    actions = np.concatenate([single_run(n)[0] for n in names], axis=1)
    obs, _, _, sr, sf = eng.advance(actions, per_step=True)
    got = eng.get_state()
    eng.close()
    for e, n in enumerate(names):
        _, o1, r1, f1, st1 = single_run(n)
        assert np.array_equal(bits(sr[:, e]), bits(r1[:, 0])) and np.array_equal(sf[:, e], f1[:, 0]), (e, n)
        assert np.array_equal(obs[e].view(np.uint32), o1[0].view(np.uint32)), (e, n)
        for k in st1:
            a, b = got[k][e], st1[k][0]
            assert np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b), (e, n, k)


# ---- reset ----
def expected_device_reset(seed, episode, vehicles_count):
    """The rule of park_begin_episode restated in NumPy on the suite's Python Philox."""
    u0, u1 = spawn_util.philox_uniform2(int(seed), 0, episode, 0)
    heading = (2.0 * np.pi) * u0
    free = list(range(parking.SPOTS))
    free.remove(parking.closest_spot(heading))
    goal = free.pop(min(int(u1 * 27), 26))
    order = []
    for i in range(vehicles_count):
        if not free:
            continue
        u = spawn_util.philox_uniform2(int(seed), 1 + i // 2, episode, 0)[i % 2]
        order.append(free.pop(min(int(u * len(free)), len(free) - 1)))
    return heading, goal, order


def assert_spawned(st, e, seed, episode, vehicles_count):
    heading, goal, order = expected_device_reset(seed, episode, vehicles_count)
    assert st["heading"][e] == heading and st["goal"][e] == goal and st["episode"][e] == episode, (e, seed, episode)
    assert list(st["order"][e, :len(order)]) == order and st["occupied"][e] == sum(1 << k for k in order), (e, seed)
    for k in ("x", "y", "speed", "acceleration", "steering", "time", "flags", "steps", "struck", "parked_crashed", "parked_impact"):
        assert st[k][e] == 0, (e, k)


@pytest.mark.parametrize("vehicles_count", [0, 10, 26])
def test_device_reset_follows_the_rule(vehicles_count):
    E = 65
    cfg = dict(parking.parking_default_config(), vehicles_count=vehicles_count)
    eng = parking.ParkEngine(parking.make_park_config(cfg, E))
    seeds = [(e * 0x9E3779B97F4A7C15 + 3) % 2 ** 64 for e in range(E)]
    obs = eng.reset(seeds=seeds)
    st = eng.get_state()
    for e in range(E):
        assert_spawned(st, e, seeds[e], 0, vehicles_count)
    gx, gy = parking.spot_position(st["goal"])
    np.testing.assert_allclose(obs[:, 2, :2], np.stack([gx, gy], 1) / 100, rtol=0, atol=1e-6)
    np.testing.assert_allclose(obs[:, 0, 4:], np.stack([np.cos(st["heading"]), np.sin(st["heading"])], 1), rtol=0, atol=1e-6)
    eng.close()


def test_autoreset_respawns_on_the_next_call():
    names = ["wall_long", "free_0", "success_in"]  # crashes at step 13, runs on, succeeds at once
    fixtures = [load(n) for n in names]
    eng = engine_for(fixtures[0], 3, autoreset=True, base_seed=77)
    eng.set_state(initial_state(fixtures))
    done_before = np.zeros(3, bool)
    episodes = np.zeros(3, int)
    for t in range(16):
        a = np.stack([z["actions"][min(t, len(z["actions"]) - 1)] for z in fixtures])[None]
        obs, reward, flags = eng.advance(a)
        st = eng.get_state()
        for e in range(3):
            if done_before[e]:  # re-spawned by this call: the new episode's first observation, no reward, no flag
                episodes[e] += 1
                assert_spawned(st, e, 77 + e, episodes[e], 0)
                assert reward[e] == 0 and flags[e] == 0
        done_before = (flags & (parking.S_TERMINATED | parking.S_TRUNCATED)) != 0
    assert episodes[0] >= 1 and episodes[1] == 0 and episodes[2] >= 1
    eng.close()


@pytest.mark.parametrize("M", [1, 64, 65])
def test_goal_reward(M):
    rng = np.random.default_rng(M)
    weights = [1, 0.3, 0, 0, 0.02, 0.02]  # (zeros among them)
    env = parking.BatchedParkingEnv({"reward_weights": weights}, num_envs=1)
    a, d = rng.normal(size=(M, 6)), rng.normal(size=(M, 6))
    want = -np.power(np.dot(np.abs(a - d), np.array(weights)), 0.5)  # parking_env.py:249-255
    np.testing.assert_allclose(env.compute_reward(a, d, {}), want, rtol=0, atol=1e-9)
    import torch
    got = env.compute_reward(torch.from_numpy(a).cuda(), torch.from_numpy(d).cuda(), {})
    assert got.is_cuda and got.dtype == torch.float64
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=1e-9)
    env.close()


@pytest.mark.parametrize("output", ["numpy", "torch"])
def test_vector_front_end_steps(output):
    from highwayenv_amd.vector import HighwayVectorEnv
    env = HighwayVectorEnv("parking-parked-v0", 5, output=output)
    obs, info = env.reset(seed=3)
    a = np.full((5, 2), 0.5, np.float32)
    if output == "torch":
        import torch
        a = torch.from_numpy(a).cuda()
    obs, reward, term, trunc, info = env.step(a)
    assert set(obs) == {"observation", "achieved_goal", "desired_goal"} and tuple(obs["observation"].shape) == (5, 6)
    assert tuple(reward.shape) == (5,) and tuple(info["is_success"].shape) == (5,) and not bool(term.any())
    if output == "torch":
        assert obs["observation"].is_cuda and reward.is_cuda and term.is_cuda
        got = env.compute_reward(obs["achieved_goal"].double(), obs["desired_goal"].double(), {})
        np.testing.assert_allclose(got.cpu().numpy(), reward.cpu().numpy(), rtol=0, atol=1e-6)  # (from the float32 observation)
    env.close()
