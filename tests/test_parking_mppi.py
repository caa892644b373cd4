"""MPPI on parking (csrc/hwy_park_mppi.h: one launch, a wavefront per environment, a candidate per lane).  The simulator's yardstick
is the advance kernel (every candidate replayed as an environment of a second engine, tests/test_parking_cem.py: replay); the
search's yardstick is the rule of DESIGN.md "MPPI on parking" in float64 NumPy, applied to the kernel's own samples and returns."""
import ctypes as C

import numpy as np
import pytest

from highwayenv_amd import parking
from tests.cem_util import NOISE_ATOL, assert_bits_equal, restate_noise, restate_samples
from tests.test_parking_cem import GAMMA, fixture_config, replay
from tests.test_parking_parity import initial_state, load, single_run

gpu = pytest.mark.gpu
NOISE_STD = 0.5
RULE_ATOL = 1e-12  # at most 256 terms of magnitude <= 1, each weight off by a few ulp of a value <= 1: about 5e-13
ENDED = parking.S_TERMINATED | parking.S_TRUNCATED


def parents():
    """Four parents on one kernel configuration: the recorded parked_10 start; the same run three steps short of its crash; an empty
    lot 7 m short of the goal spot at 4 m/s (it coasts into the goal at the third step); parked_10 past its crash (struck, done)."""
    p10, out = load("parked_10"), load("success_out")
    st = initial_state([p10, p10, out, p10])
    for k, v in zip(parking.EGO_FIELDS[:6], p10["ego"][8]):
        st[k][1] = v
    st["x"][2], st["y"][2], st["heading"][2], st["speed"][2] = 2.0, 7.0, np.pi / 2, 4.0
    for k, v in single_run("parked_10")[4].items():
        st[k][3] = v[0]
    return st


def colour(z, beta):
    """n[0] = z[0]; n[k] = beta * n[k-1] + beta_c * z[k] along axis -2, one rounded operation per statement."""
    beta_c = np.sqrt(np.float64(1.0) - np.float64(beta) * np.float64(beta))
    n = np.array(z, np.float64)
    for k in range(1, n.shape[-2]):
        t1 = beta * n[..., k - 1, :]
        t2 = beta_c * z[..., k, :]
        n[..., k, :] = t1 + t2
    return n


@gpu
@pytest.mark.parametrize("B,K,I,alpha,beta,temperature,warm", [
    (1, 1, 1, 1.0, 0.0, 0.1, False),      # a single, unperturbed candidate
    (65, 3, 2, 1.0, 0.0, 0.1, False),     # a second pass with one live lane; 6 columns in groups of 8
    (128, 32, 2, 1.0, 0.3, 0.1, False),   # 64 columns (one lane group) and the LDS cap
    (256, 16, 1, 1.0, 0.0, 0.5, False),   # four full passes
    (96, 5, 3, 0.5, 0.7, 0.1, True),
    (64, 8, 2, 1.0, 0.0, 1e-6, False)])   # the weights collapse onto the best candidate
def test_plan_mppi_is_the_restated_search(B, K, I, alpha, beta, temperature, warm):
    state, seed = parents(), 0x3A990000 + B
    E = len(state["x"])
    env = parking.BatchedParkingEnv(fixture_config(), num_envs=E)
    env.set_state(state)
    before = env.get_state()
    init_mean = np.random.default_rng(K).uniform(-0.3, 0.3, (E, K, 2)) if warm else None
    action, det = env.plan_mppi(B, I, K, GAMMA, NOISE_STD, temperature, beta, alpha, seed=seed, init_mean=init_mean,
                                return_details=True, debug=True)
    after = env.get_state()
    env.close()
    for k in before:
        assert_bits_equal(after[k], before[k], f"parent {k}")
    white = restate_noise(seed, E, B, K, 2, I)
    np.testing.assert_allclose(det["noise"], colour(white, beta), rtol=0, atol=NOISE_ATOL)
    assert not det["noise"][:, :, 0].any()  # candidate 0 is the mean, exactly
    hist = det["mean_history"]
    assert_bits_equal(hist[0], np.zeros((E, K, 2)) if init_mean is None else init_mean, "the first mean")
    struck = success = early = False
    worst = 0.0
    for i in range(I):
        x, ret = det["samples"][i], det["returns"][i]
        assert_bits_equal(x, restate_samples(hist[i], np.full((E, K, 2), NOISE_STD), det["noise"][i]), f"samples {i}")
        want_ret, _, sf, final = replay(state, x)
        assert_bits_equal(ret, want_ret, f"returns {i}")
        struck |= bool((final["struck"].reshape(E, B)[1] != 0).any())
        success |= bool((sf[2] & parking.S_SUCCESS).any())
        early |= bool((sf[1:3, :, :-1] & ENDED).any())
        a = (ret - ret.max(axis=1, keepdims=True)) / temperature
        w = np.where(a > -700.0, np.exp(a), 0.0)
        eta = w.sum(axis=1)
        m = np.einsum("eb,ebkc->ekc", w, x.astype(np.float64)) / eta[:, None, None]
        worst = max(worst, np.abs(det["weights"][i] - w).max(), np.abs(hist[i + 1] - (alpha * m + (1.0 - alpha) * hist[i])).max())
        if temperature < 1e-3:  # one weight of 1 and the rest flushed: the mean IS the best sample
            alone = (w != 0).sum(axis=1) == 1
            assert alone.any() and (det["weights"][i] == 0).any()
            top = x[np.arange(E), ret.argmax(axis=1)].astype(np.float64)
            assert np.array_equal(hist[i + 1][alone], top[alone])
    print(f"largest deviation from the float64 rule (B={B}, K={K}): {worst:.3e}")
    assert worst <= RULE_ATOL
    assert_bits_equal(det["mean"], hist[-1], "mean")
    assert_bits_equal(action, np.clip(hist[-1][:, 0], -1.0, 1.0).astype(np.float32), "action")
    assert_bits_equal(det["best_return"], det["returns"].max(axis=(0, 2)), "best_return")
    np.testing.assert_allclose(det["weights_ess"], eta ** 2 / (w * w).sum(axis=1), rtol=RULE_ATOL, atol=0)
    if K >= 4 and not warm:  # the candidate that is the zero mean strikes from parent 1 and coasts into the goal from parent 2
        assert struck, "no candidate strikes a parked vehicle"
        assert success, "no candidate succeeds"
        assert early, "no candidate ends early"


@gpu
def test_front_ends():
    import torch
    from highwayenv_amd.vector import HighwayVectorEnv
    got = {}
    for output in ("torch", "numpy"):
        env = HighwayVectorEnv("parking-v0", 5, output=output)
        env.reset(seed=3)
        got[output] = env.plan_mppi(seed=11)
        if output == "torch":
            assert got[output].is_cuda and got[output].dtype == torch.float32 and tuple(got[output].shape) == (5, 2)
            got[output] = got[output].cpu().numpy()  # (a copy: step's launch comes after it on the stream)
        assert tuple(env.step(env.plan_mppi())[1].shape) == (5,)
        env.close()
    assert_bits_equal(got["torch"], got["numpy"], "the two front ends")
    one = parking.ParkingEnv()
    one.reset(seed=3)
    assert one.plan_mppi().shape == (2,)
    one.close()


@pytest.mark.parametrize("change", [{"temperature": 0.0}, {"temperature": -1.0}, {"temperature": np.nan}, {"beta": 1.0}, {"population": 257},
                                    {"population": 241, "horizon": 17}, {"iterations": 17}])
def test_parameters_outside_the_caps_raise_before_the_device(change, monkeypatch):
    monkeypatch.setattr(parking, "ParkEngine", lambda *a, **k: pytest.fail("the device was touched"))
    with pytest.raises(ValueError):
        parking.BatchedParkingEnv(num_envs=2).plan_mppi(**change)


@pytest.mark.parametrize("field,value,reason", [("struct_size", 8, b"struct_size"), ("temperature", 0.0, b"temperature")])
def test_c_entry_point_refuses_bad_parameters_without_a_handle(field, value, reason):
    lib = parking.load()
    mppi = parking.park_mppi_params(64, 3, 8, 0.9, 0.5, 0.1, 0.0, 1.0, 0)
    setattr(mppi, field, value)
    action = np.zeros((2, 2), np.float32)
    assert lib.hwy_park_mppi_plan(None, C.addressof(mppi), None, action.ctypes.data, *([None] * 8)) == 1
    assert reason in lib.hwy_park_last_error(None)
