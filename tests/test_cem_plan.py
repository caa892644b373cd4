"""plan_cem against the plain-NumPy restatement of tests/cem_util.py, on the CPU emulation and on the GPU: given the engine's own
noise, the samples and the elite set of every iteration, the mean and std after the last refit, the best sequence, its return and
the action are the restatement's bit for bit.
The noise itself is held to a float64 NumPy Box-Muller on the project's Python Philox within cu.NOISE_ATOL."""
import numpy as np
import pytest

from highwayenv_amd import _abi
from tests import cem_util as cu

# B in {1, 5, 64, 65} (65: the second lane pass of the refit and of the score kernel), M in {1, B} and in between, K in {1, 3},
# size 1 and 2, alpha 0.5, init_mean given, I = 1 and 3
CASES = [
    dict(population=1, elites=1, horizon=1, size=2, iterations=1),
    dict(population=5, elites=2, horizon=3, size=2, iterations=3),
    dict(population=5, elites=5, horizon=3, size=1, iterations=3, alpha=0.5, init_mean=True),
    dict(population=5, elites=1, horizon=1, size=1, iterations=1),
    dict(population=64, elites=8, horizon=1, size=2, iterations=3),
    dict(population=64, elites=64, horizon=3, size=2, iterations=1, alpha=0.5),
    dict(population=65, elites=1, horizon=3, size=2, iterations=1),
    dict(population=65, elites=64, horizon=1, size=1, iterations=3, alpha=0.5, init_mean=True),
    dict(population=65, elites=65, horizon=1, size=2, iterations=3),
]
GAMMA, SEED, E = 0.9, 1234, 3
_draws = {}   # backend -> [(engine's noise, restated noise)] of every plan of this module, for the tolerance's measurement


def _id(c):
    return "B{population}-M{elites}-K{horizon}-s{size}-I{iterations}".format(**c) + ("-a" if "alpha" in c else "") + ("-m" if c.get("init_mean") else "")


def run_case(backend, c, env=None, init_mean=None, init_std=0.5, seed=SEED):
    env = env or cu.make_env(backend, E, size=c["size"])
    cem = _abi.cem_params(c["population"], c["elites"], c["iterations"], c["horizon"], GAMMA, init_std, 0.05, c.get("alpha", 1.0), seed)
    if c.get("init_mean") and init_mean is None:
        init_mean = np.random.default_rng(5).uniform(-0.8, 0.8, size=(env.num_envs, c["horizon"], c["size"]))
    snap = cu.parent_snapshot(env)
    action, det = env.plan_cem(population=cem.population, elites=cem.elites, iterations=cem.iterations, horizon=cem.horizon, gamma=GAMMA,
                               init_std=init_std, min_std=0.05, alpha=cem.alpha, seed=seed, init_mean=init_mean, return_details=True,
                               debug=True)
    cu.assert_parent_unchanged(env, snap)
    want = cu.restate_plan(det["noise"], lambda x: env.score_sequences_continuous(x, gamma=GAMMA), cem, init_mean)
    # every iteration's elite set, read out of the engine, is the restatement's
    assert det["elites"].shape == (cem.iterations, env.num_envs, cem.elites) and det["elites"].dtype == np.int32
    np.testing.assert_array_equal(det["elites"], np.asarray(want["elites"], np.int32), err_msg="elites")
    return env, cem, action, det, want


@pytest.mark.parametrize("case", CASES, ids=_id)
@pytest.mark.parametrize("backend", cu.BACKENDS)
def test_plan_equals_the_restatement_bit_for_bit(backend, case):
    env, cem, action, det, want = run_case(backend, case)
    I, B, K, size = cem.iterations, cem.population, cem.horizon, case["size"]
    assert action.shape == (E, size) and action.dtype == np.float32
    assert det["noise"].shape == (I, E, B, K, size) and (det["noise"][:, :, 0] == 0).all()   # branch 0 IS the mean
    for k in ("samples", "mean", "std", "best_sequence", "best_return"):
        cu.assert_bits_equal(det[k], want[k], k)
    cu.assert_bits_equal(action, want["action"], "action")
    cu.assert_bits_equal(action, det["best_sequence"][:, 0], "the action is step 0 of the best sequence")
    # the noise is the float64 NumPy Box-Muller on the Python Philox
    z = cu.restate_noise(SEED, E, B, K, size, I)
    _draws.setdefault(backend, []).append(np.abs(det["noise"] - z).max())
    print(f"{backend}: largest |engine normal - NumPy normal| of this plan: {_draws[backend][-1]:.3g}")
    np.testing.assert_allclose(det["noise"], z, rtol=0, atol=cu.NOISE_ATOL)
    assert np.abs(det["noise"]).max() <= 8.6
    # best_return is score_sequences_continuous(best_sequence), recomputed; it is at least the init_mean sequence's return (branch 0
    # of iteration 0) and does not decrease over the iterations
    again = env.score_sequences_continuous(det["best_sequence"][:, None], gamma=GAMMA)[:, 0]
    cu.assert_bits_equal(det["best_return"], again, "best_return recomputed")
    per_it = np.stack(want["best_return_per_iteration"])
    assert (det["best_return"] >= want["returns"][0][:, 0]).all() and (np.diff(per_it, axis=0) >= 0).all()
    env.close()


@pytest.mark.parametrize("backend", cu.BACKENDS)
def test_zero_init_std_everything_ties(backend):
    """init_std = 0: every sample is the mean, every return ties, the elites are the M lowest branches (the refit of equal samples is
    exact: mean' = the sample, s = 0) and std becomes min_std; the best branch is branch 0."""
    c = dict(population=5, elites=2, horizon=3, size=2, iterations=1, init_mean=True)
    env, cem, action, det, want = run_case(backend, c, init_std=0.0)
    assert (det["samples"] == det["samples"][:, :, :1]).all()
    assert all((el == np.arange(2)).all() for it in want["elites"] for el in it)
    assert (det["std"] == 0.05).all()
    for k in ("samples", "mean", "std", "best_sequence", "best_return"):
        cu.assert_bits_equal(det[k], want[k], k)
    cu.assert_bits_equal(det["best_sequence"], det["samples"][0][:, 0], "the earliest iteration, the lowest branch")
    env.close()


@pytest.mark.parametrize("backend", cu.BACKENDS)
def test_equal_returns_break_toward_the_lowest_branch(backend):
    """An ego far off the road earns exactly 0 whatever it does (the reward is multiplied by on_road): every return ties while the
    samples differ.  The elites are the M LOWEST branches and the best sequence is branch 0's of the first iteration."""
    env = cu.make_env(backend, E)
    st = env.get_state()
    st["y"][:, env._hcfg.agent_index[0]] = -40.0
    env.set_state(st)
    c = dict(population=5, elites=2, horizon=3, size=2, iterations=3)
    env, cem, action, det, want = run_case(backend, c, env=env)
    assert all((r == 0.0).all() for r in want["returns"]) and (det["samples"][0][:, 1] != det["samples"][0][:, 4]).any()
    assert all((el == np.arange(2)).all() for it in want["elites"] for el in it)
    for k in ("samples", "mean", "std", "best_sequence", "best_return"):
        cu.assert_bits_equal(det[k], want[k], k)
    cu.assert_bits_equal(det["best_sequence"], det["samples"][0][:, 0], "the earliest iteration, the lowest branch")
    assert (det["best_return"] == 0.0).all()
    env.close()


@pytest.mark.parametrize("backend", cu.BACKENDS)
def test_a_terminated_branch(backend):
    """From one step before the ego of tests/golden/cem/cem_respawn runs into its leader, around full throttle: some but not all
    sequences end inside the horizon; an ended branch is absorbing in the returns the refit ranks."""
    g = cu.CemGolden("cem_respawn")
    env = cu.env_class(backend)(g.config, num_envs=g.E)
    env.reset(seed=0)
    env._engine.set_state(g.prev_state())
    env._engine.set_controls(*g.controls_of("prev", env._hcfg))
    c = dict(population=5, elites=2, horizon=3, size=2, iterations=3)
    mean = np.broadcast_to(np.array([1.0, 0.0]), (g.E, 3, 2)).copy()
    env, cem, action, det, want = run_case(backend, c, env=env, init_mean=mean, init_std=1.0)
    _, d0 = env.score_sequences_continuous(det["samples"][0], gamma=GAMMA, return_details=True)
    ended = d0["terminated"].any(axis=2)
    print("ended branches per environment:", ended.sum(axis=1))
    assert ended.any() and not ended.all()
    for k in ("samples", "mean", "std", "best_sequence", "best_return"):
        cu.assert_bits_equal(det[k], want[k], k)
    cu.assert_bits_equal(action, want["action"], "action")
    env.close()


@pytest.mark.parametrize("backend", cu.BACKENDS)
def test_seeds_and_environment_order(backend):
    """The same seed gives the same plan on two calls and, environment by environment, whatever the batch the environment sits in
    (the counter holds the environment INDEX: a batch of the same states in another order draws other noise for a state, the same
    noise for an index); another seed gives other samples."""
    kw = dict(population=5, elites=2, iterations=3, horizon=3, gamma=GAMMA, return_details=True, debug=True)
    env = cu.make_env(backend, E)
    a1, d1 = env.plan_cem(seed=9, **kw)
    a2, d2 = env.plan_cem(seed=9, **kw)
    cu.assert_bits_equal(a1, a2)
    for k in d1:
        cu.assert_bits_equal(d1[k], d2[k], k)
    _, d3 = env.plan_cem(seed=10, **kw)
    assert (d3["samples"][:, :, 1:] != d1["samples"][:, :, 1:]).any() and (d3["noise"][:, :, 1:] != d1["noise"][:, :, 1:]).all()
    # the environments in reverse order: the noise of index e is unchanged, so states that swap places swap nothing of the noise
    st = env.get_state()
    rev = cu.make_env(backend, E)
    rev.set_state({k: np.ascontiguousarray(v[::-1]) for k, v in st.items()})
    acc, steer = env._engine.get_controls()
    rev._engine.set_controls(acc[::-1].copy(), steer[::-1].copy())
    _, d4 = rev.plan_cem(seed=9, **kw)
    cu.assert_bits_equal(d4["noise"], d1["noise"], "noise by environment index")
    # ... and the middle environment (index 1 in both) plans the same
    cu.assert_bits_equal(d4["best_sequence"][1], d1["best_sequence"][1])
    # the default seed: no two decisions share noise, with or without a step between them, and a reset(seed) replays them
    _, e1 = env.plan_cem(**kw)
    _, e1b = env.plan_cem(**kw)
    env.step_continuous(np.zeros(2, np.float32))
    _, e2 = env.plan_cem(**kw)
    for a, b in ((e1, e1b), (e1, e2), (e1b, e2)):
        assert (a["noise"][:, :, 1:] != b["noise"][:, :, 1:]).all()
    env.reset(seed=11)       # (make_env's seed: the explicit-seed calls above drew nothing from the default stream)
    _, f1 = env.plan_cem(**kw)
    cu.assert_bits_equal(f1["noise"], e1["noise"], "the first default-seed decision after reset(seed=11)")
    env.close(), rev.close()


def test_the_noise_tolerance_is_four_times_the_measured_difference():
    """cu.NOISE_ATOL against the largest difference on the CPU emulation: over 1e5 draws of the sample kernel alone and over the
    plans of this module that ran before (profiles/cem.md records the figure)."""
    from tests.emu import emu_cem
    cp = _abi.continuous_params({"type": "DiscreteAction"})
    z = emu_cem.cem_sample(cp, _abi.cem_params(1024, 1, 1, 25, GAMMA, 0.5, 0.05, 1.0, SEED), 2)["noise"]
    worst = max([np.abs(z - cu.restate_noise(SEED, 2, 1024, 25, 2, 1)[0]).max()] + _draws.get("emu", []))
    print(f"largest |engine normal - NumPy normal| on the emulation: {worst:.3g}; tolerance {cu.NOISE_ATOL:.3g}")
    assert worst * 4 <= cu.NOISE_ATOL
