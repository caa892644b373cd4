"""Device-side reset (hwy_reset / auto-reset) against the spawn RULE pinned to the reference.

The device spawn draws from Philox-4x32-10 (counter-based, one stream per env), NOT numpy's PCG64
stream; what must match the reference is the rule that turns draws into traffic
(Vehicle.create_random, highway_env/vehicle/kinematics.py:50-104).  ``spawn.spawn_from_draws`` is
that rule, verified against the reference's own reset states in tests/test_spawn.py; here the
kernel is checked against it on the same Philox uniforms, computed independently in Python
(tests/spawn_util.py; every kernel path and size: tests/test_spawn_paths.py).
"""
import numpy as np
import pytest

from highwayenv_amd import _abi
from oracle import oracle
from tests.backends import BACKENDS, make_engine
from tests.spawn_util import assert_spawn_equal, expected_state


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("fast,controlled,lane_id", [(True, 1, -1), (False, 1, 2), (False, 3, -1)])
def test_device_reset_follows_the_reference_spawn_rule(backend, fast, controlled, lane_id):
    cfg_d = _abi.highway_fast_default_config() if fast else _abi.highway_default_config()
    cfg_d.update({"vehicles_count": 24, "lanes_count": 4, "controlled_vehicles": controlled})
    E = 5
    cfg = _abi.make_config(cfg_d, E, fast=fast)
    eng = make_engine(backend, cfg)
    seeds = np.array([3, 2**40 + 17, 99, 12345678901234567, 0], np.uint64)
    obs = eng.reset(seeds=seeds, ego_spacing=1.7, vehicles_density=1.3, initial_lane_id=lane_id)
    got = eng.get_state()
    want = expected_state(cfg, seeds, 0, 1.7, 1.3, lane_id)
    assert_spawn_equal(got, want)
    assert (got["time"] == 0).all()
    # first observation == KinematicObservation of the spawned state
    np.testing.assert_allclose(obs, oracle.observe(cfg, want), rtol=0, atol=1e-6)
    # x strictly increasing in creation order (every vehicle is placed ahead of the previous ones)
    assert (np.diff(got["x"], axis=1) > 0).all()
    eng.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_masked_reset_leaves_other_envs_untouched(backend):
    cfg_d = _abi.highway_fast_default_config()
    cfg = _abi.make_config(cfg_d, 4, fast=True)
    eng = make_engine(backend, cfg)
    eng.reset(seeds=np.arange(4, dtype=np.uint64))
    eng.step(np.ones((4, 1), np.int32))
    before = eng.get_state()
    eng.reset(seeds=np.arange(10, 14, dtype=np.uint64), mask=np.array([0, 1, 0, 1], np.uint8))
    after = eng.get_state()
    for k in before:
        np.testing.assert_array_equal(after[k][[0, 2]], before[k][[0, 2]], err_msg=k)
    want = expected_state(cfg, np.arange(10, 14), 0, 2.0, 1.0, -1)
    assert_spawn_equal(after, want, rows=[1, 3])
    assert (after["time"][[1, 3]] == 0).all() and (after["time"][[0, 2]] == 1).all()
    eng.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_autoreset_next_step_semantics(backend):
    """gymnasium vector 'next-step' auto-reset: the step after terminated|truncated re-spawns the env
    (new Philox episode), ignores the action, returns the reset observation with reward 0 and both
    flags False; envs that are not done keep stepping exactly like the oracle."""
    cfg_d = _abi.highway_fast_default_config()
    cfg_d.update({"duration": 3, "vehicles_count": 12})
    E = 6
    cfg = _abi.make_config(cfg_d, E, fast=True)
    eng = make_engine(backend, cfg)
    base = 4242
    eng.reset(seeds=np.uint64(base) + np.arange(E, dtype=np.uint64), ego_spacing=1.5)
    eng.set_autoreset(True, base_seed=base, ego_spacing=1.5, vehicles_density=1.0)
    ref = eng.get_state()
    episode = np.zeros(E, np.int64)
    done_prev = np.zeros(E, bool)
    rng = np.random.default_rng(0)
    n_resets = 0
    for t in range(9):
        acts = rng.integers(0, 5, size=(E, 1)).astype(np.int32)
        obs, reward, term, trunc, info = eng.step(acts)
        # oracle on the envs that were live; fresh spawn for the ones that were done
        o2, r2, te2, tr2, _ = oracle.step(cfg, ref, acts)
        for e in np.nonzero(done_prev)[0]:
            episode[e] += 1
            fresh = expected_state(cfg, [base + e], int(episode[e]), 1.5, 1.0, -1)
            for k in ref:
                ref[k][e] = fresh[k][0] if k != "time" else 0.0
            sub = _abi.make_config(cfg_d, 1, fast=True)
            o2[e] = oracle.observe(sub, fresh)[0]
            r2[e], te2[e], tr2[e] = 0.0, False, False
            n_resets += 1
        np.testing.assert_array_equal(term, te2, err_msg=f"step {t}")
        np.testing.assert_array_equal(trunc, tr2, err_msg=f"step {t}")
        np.testing.assert_allclose(reward, r2, rtol=0, atol=1e-9, err_msg=f"step {t}")
        np.testing.assert_allclose(obs, o2, rtol=0, atol=1e-6, err_msg=f"step {t}")
        got = eng.get_state()
        np.testing.assert_allclose(got["x"], ref["x"], rtol=0, atol=1e-7)
        np.testing.assert_array_equal(got["time"], ref["time"])
        done_prev = term | trunc
    assert n_resets >= E  # duration 3 => every env was truncated and re-spawned at least once
    eng.close()
