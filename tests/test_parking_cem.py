"""Sampling MPC on parking (csrc/hwy_park_cem.h: one launch, a wavefront per environment, a candidate per lane).  The simulator's
yardstick is the project's own advance kernel (tests/test_parking_parity.py holds it to the reference): every candidate is replayed
as an environment of a second engine.  The search's yardstick is the NumPy restatement of tests/cem_util.py."""
import ctypes as C

import numpy as np
import pytest

from highwayenv_amd import parking
from tests.cem_util import NOISE_ATOL, assert_bits_equal, fold_returns, restate_noise, restate_plan
from tests.test_parking_parity import BATCH_STEPS, DEFAULT_GROUP, initial_state, load, single_run

gpu = pytest.mark.gpu
GAMMA = 0.9


def replay(parent_state, samples, config=None, gamma=GAMMA):
    """samples f32 [E, B, K, 2] stepped by the advance kernel: a second engine of E * B environments without autoreset, set to the
    tiled parent state.  -> (returns [E, B], reward [E, B, K], flags [E, B, K], the final state)."""
    E, B, K, _ = samples.shape
    eng = parking.ParkEngine(parking.make_park_config(config or fixture_config(), E * B))
    eng.set_state({k: np.repeat(v, B, axis=0) for k, v in parent_state.items()})
    _, _, _, sr, sf = eng.advance(np.ascontiguousarray(samples.reshape(E * B, K, 2).transpose(1, 0, 2)), per_step=True)
    final = eng.get_state()
    eng.close()
    sr, sf = sr.T.reshape(E, B, K), sf.T.reshape(E, B, K)
    return fold_returns(sr, (sf & parking.S_TERMINATED) != 0, (sf & parking.S_TRUNCATED) != 0, gamma), sr, sf, final


def fixture_config():
    import json
    return dict(parking.parking_default_config(), **json.loads(str(load(DEFAULT_GROUP[0])["config_json"])))


def check_scores(state, candidates):
    """score_sequences from ``state`` against the replay, bit for bit; the parent is left as it was.  -> the replay."""
    env = parking.BatchedParkingEnv(fixture_config(), num_envs=candidates.shape[0])
    env.set_state(state)
    before = env.get_state()
    ret, det = env.score_sequences(candidates, gamma=GAMMA, return_details=True)
    after = env.get_state()
    env.close()
    want = replay(state, candidates)
    assert_bits_equal(ret, want[0], "returns")
    assert_bits_equal(det["reward"], want[1], "step rewards")
    for key, bit in (("terminated", parking.S_TERMINATED), ("truncated", parking.S_TRUNCATED), ("is_success", parking.S_SUCCESS),
                     ("crashed", parking.S_CRASHED)):
        assert np.array_equal(det[key], (want[2] & bit) != 0), key
    for k in before:
        assert_bits_equal(after[k], before[k], f"parent {k}")
    return want


@gpu
@pytest.mark.parametrize("B", [1, 64, 65])  # one lane, a full pass, a second (partial) pass
def test_score_sequences_is_the_advance_kernel(B):
    K, E = BATCH_STEPS, len(DEFAULT_GROUP)
    candidates = np.random.default_rng(B).uniform(-1, 1, (E, B, K, 2)).astype(np.float32)
    candidates[:, 0] = np.stack([single_run(n)[0][:, 0] for n in DEFAULT_GROUP])  # each fixture's own actions, zero-padded to K
    _, _, sf, final = check_scores(initial_state([load(n) for n in DEFAULT_GROUP]), candidates)
    crashed = (np.asarray(final["flags"]) & parking.F_CRASHED) != 0
    assert (crashed & (final["struck"] == 0)).any(), "no candidate crashes into a wall"
    assert (final["struck"] != 0).any(), "no candidate strikes a parked vehicle"
    assert (sf & parking.S_SUCCESS).any(), "no candidate succeeds"


@gpu
def test_score_sequences_from_a_parent_that_is_already_struck():
    state = single_run("parked_10")[4]  # past its crash, autoreset off: done, a struck body in the planes
    assert state["struck"][0] != 0 and state["flags"][0] & parking.F_DONE
    check_scores(state, np.random.default_rng(7).uniform(-1, 1, (1, 65, 8, 2)).astype(np.float32))


@gpu
@pytest.mark.parametrize("B,M,K,I,alpha,warm", [(64, 8, 8, 3, 1.0, False), (65, 5, 3, 2, 0.7, True), (7, 7, 1, 1, 1.0, False),
                                                (256, 16, 16, 2, 1.0, False)])
def test_plan_cem_is_the_restated_search(B, M, K, I, alpha, warm):
    E, seed = 3, 0x5EED0000 + B
    env = parking.BatchedParkingEnvParkedVehicles(num_envs=E, spawn_mode="device")
    env.reset(seed=5)
    state = env.get_state()
    init_mean = np.random.default_rng(K).uniform(-0.5, 0.5, (E, K, 2)) if warm else None
    action, det = env.plan_cem(B, M, I, K, gamma=GAMMA, alpha=alpha, seed=seed, init_mean=init_mean, return_details=True, debug=True)
    after = env.get_state()
    env.close()
    for k in state:
        assert_bits_equal(after[k], state[k], f"parent {k}")
    np.testing.assert_allclose(det["noise"], restate_noise(seed, E, B, K, 2, I), rtol=0, atol=NOISE_ATOL)
    cem = parking.park_cem_params(B, M, I, K, GAMMA, 0.5, 0.05, alpha, seed)
    want = restate_plan(det["noise"], lambda x: replay(state, x, env.config)[0], cem, init_mean)
    assert_bits_equal(det["samples"], want["samples"], "samples")
    assert_bits_equal(det["returns"], np.stack(want["returns"]), "returns")
    assert_bits_equal(det["elites"], np.asarray(want["elites"], np.int32), "elites")
    for k in ("mean", "std", "best_sequence", "best_return"):
        assert_bits_equal(det[k], want[k], k)
    assert_bits_equal(action, want["action"], "action")


@gpu
def test_front_ends():
    import torch
    from highwayenv_amd.vector import HighwayVectorEnv
    got = {}
    for output in ("torch", "numpy"):
        env = HighwayVectorEnv("parking-v0", 5, output=output)
        env.reset(seed=3)
        got[output] = env.plan_cem(seed=11)
        if output == "torch":
            assert got[output].is_cuda and got[output].dtype == torch.float32 and tuple(got[output].shape) == (5, 2)
            got[output] = got[output].cpu().numpy()  # (a copy: step's launch comes after it on the stream)
        assert tuple(env.step(env.plan_cem())[1].shape) == (5,)
        env.close()
    assert_bits_equal(got["torch"], got["numpy"], "the two front ends")
    one = parking.ParkingEnv()
    one.reset(seed=3)
    assert one.plan_cem().shape == (2,) and one.score_sequences(np.zeros((4, 3, 2), np.float32)).shape == (4,)
    one.close()


@pytest.mark.parametrize("change", [{"population": 0}, {"population": 257}, {"elites": 0}, {"elites": 65}, {"horizon": 0}, {"horizon": 33},
                                    {"population": 256, "horizon": 32}, {"iterations": 0}, {"iterations": 17}, {"gamma": np.inf},
                                    {"init_std": -1.0}, {"min_std": np.nan}, {"alpha": 1.5}])
def test_parameters_outside_the_caps_raise_before_the_device(change, monkeypatch):
    monkeypatch.setattr(parking, "ParkEngine", lambda *a, **k: pytest.fail("the device was touched"))
    with pytest.raises(ValueError):
        parking.BatchedParkingEnv(num_envs=2).plan_cem(**change)
    with pytest.raises(ValueError):
        parking.BatchedParkingEnv(num_envs=2).score_sequences(np.zeros((257, 2, 2), np.float32))
    with pytest.raises(MemoryError, match="106496 bytes"):
        parking.BatchedParkingEnv(num_envs=2, max_plan_bytes=100000).plan_cem()


@gpu
def test_c_entry_point_refuses_a_sample_table_beyond_lds():
    eng = parking.ParkEngine(parking.make_park_config(parking.parking_default_config(), 2))
    cem = parking.park_cem_params(64, 8, 1, 8, 0.9, 0.5, 0.05, 1.0, 0)
    cem.population, cem.horizon = 256, 32
    action = np.zeros((2, 2), np.float32)
    rc = eng.lib.hwy_park_cem_plan(eng.h, C.addressof(cem), None, action.ctypes.data, *([None] * 8))
    assert rc == 1 and b"population * horizon" in eng.lib.hwy_park_last_error(eng.h)
    eng.close()
