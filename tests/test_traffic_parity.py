"""The LinearVehicle family's kernels (the LinearTraffic policy of the one-wavefront kernel, hwy_wave.h: hwy_step_wave_linear_kernel
/ hwy_rollout_wave_linear_kernel for N <= 64, and of the workgroup kernel, hwy_device.h: hwy_step_linear_kernel /
hwy_rollout_linear_kernel / hwy_reset_linear_kernel) against the unmodified reference's fixtures
(tests/golden/traffic), on the CPU emulation of the kernel source (``emu``) and on the MI355X (``hip``).

Here the reference's own traces are the yardstick; the C oracle restates the Linear model too (pinned to these fixtures by
tests/test_oracle_golden_families.py) and is the yardstick beyond their shapes (tests/test_fuzz_configs.py, tests/test_families_edge_cases.py).  Knife edges: a discrete
decision that sits within rounding of its threshold may go the other way under another libm or BLAS (np.dot's summation order
is not specified); such frames are COUNTED per fixture and capped at the counts measured on both backends, never dropped."""
import numpy as np
import pytest

from highwayenv_amd import _abi, spawn
from tests.golden_util import assert_state_close
from tests.traffic_util import BACKENDS, FIXTURES, TrafficGolden, make_engine

# teacher-forced frames whose discrete outcome (lane / target lane / flags) differs from the reference's, per fixture: the cap
KNIFE_FRAMES = {name: 0 for name in FIXTURES}


def _engine(backend, g: TrafficGolden, envs=None):
    cfg = g.hwy_config(len(envs) if envs is not None else None)
    return make_engine(backend, cfg)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", [n for n in FIXTURES if n != "crash_many_linear"])
def test_teacher_forced_frames(backend, name):
    """Every recorded frame from the reference's own previous frame: positions, speeds, headings at 1e-9, lanes and flags exact."""
    g = TrafficGolden(name)
    envs = list(range(g.frames_for))
    eng = _engine(backend, g, envs)
    behavior = g.behavior[envs]
    edges = 0
    n_frames = g.steps * g.T
    for j in range(n_frames):
        t, f = divmod(j, g.T)
        prev = g.state("init", envs=envs) if j == 0 else g.state("frame", j - 1, envs=envs)
        eng.set_state(prev)
        eng.set_behavior(behavior)
        acts = np.asarray(g.actions[t], np.int32).reshape(g.E, g.A)[envs] if f == 0 else None
        eng.step_frames(acts, 1)
        got, want = eng.get_state(), g.state("frame", j, envs=envs)
        discrete_ok = all(np.array_equal(got[k], want[k]) for k in ("lane", "target_lane", "flags"))
        if not discrete_ok:
            edges += 1
            continue
        assert_state_close(got, want, atol=1e-9, what=f"{name} frame {j}")
    eng.close()
    assert edges <= KNIFE_FRAMES[name], f"{name}: {edges} knife-edge frames"


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", [n for n in FIXTURES if n != "linear_n100"])
def test_wave_and_workgroup_kernels_bit_identical(backend, name):
    """N <= 64: the one-wavefront kernel (the engine's choice) and the workgroup kernel (tune_block_kernel = 1) give the same
    simulation, bit for bit, over the whole fixture: every state plane, reward, terminated / truncated / crashed.  The f32
    observation may be one f32 rounding apart (the one-wavefront kernel's observe multiplies by host-computed reciprocals of the
    feature ranges, StepParams::inv_*, like for IDM traffic; tests/test_wide_kernel.py compares the states the same way): 1e-6."""
    g = TrafficGolden(name)
    engines = [make_engine(backend, g.hwy_config(tuning={"block_kernel": b})) for b in (0, 1)]
    for eng in engines:
        eng.set_state(g.state("init"))
        eng.set_behavior(g.behavior)
    for t in range(g.steps):
        outs = [eng.step(g.actions_at(t)) for eng in engines]
        np.testing.assert_allclose(outs[0][0], outs[1][0], rtol=0, atol=1e-6, err_msg=f"{name} step {t}: obs")
        for j in (1, 2, 3):
            np.testing.assert_array_equal(outs[0][j], outs[1][j], err_msg=f"{name} step {t} output {j}")
        np.testing.assert_array_equal(outs[0][4]["crashed"], outs[1][4]["crashed"])
    sa, sb = engines[0].get_state(), engines[1].get_state()
    for key in _abi.STATE_F64 + _abi.STATE_I32:
        np.testing.assert_array_equal(sa[key], sb[key], err_msg=key)
    for eng in engines:
        eng.close()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", FIXTURES)
def test_free_running_episodes(backend, name):
    """Whole episodes from the reference's initial state: obs 1e-6, reward 1e-9, crashed / terminated / truncated and lanes exact,
    each environment up to and including its first terminated step (afterwards the reference keeps stepping a finished one)."""
    g = TrafficGolden(name)
    eng = _engine(backend, g)
    eng.set_state(g.state("init"))
    eng.set_behavior(g.behavior)
    z = g.z
    alive = np.ones(g.E, bool)
    for t in range(g.steps):
        obs, reward, term, trunc, info = eng.step(g.actions_at(t))
        got = eng.get_state()
        rows = np.flatnonzero(alive)
        for k in ("lane", "target_lane"):
            np.testing.assert_array_equal(got[k][rows], z["step_" + k][t][rows], err_msg=f"{name} step {t}: {k}")
        want_obs = z["obs"][t].reshape(obs.shape)
        np.testing.assert_allclose(obs[rows], want_obs[rows], rtol=0, atol=1e-6, err_msg=f"{name} step {t}: obs")
        np.testing.assert_allclose(reward[rows, 0], z["reward"][t][rows], rtol=0, atol=1e-9, err_msg=f"{name} step {t}: reward")
        np.testing.assert_array_equal(term[rows], z["terminated"][t][rows].astype(bool), err_msg=f"{name} step {t}: terminated")
        np.testing.assert_array_equal(trunc[rows], z["truncated"][t][rows].astype(bool), err_msg=f"{name} step {t}: truncated")
        np.testing.assert_array_equal(info["crashed"][rows, 0], z["step_crashed"][t][rows, g.hwy_config().agent_index[0]] != 0)
        alive &= ~np.asarray(term, bool)
    eng.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_final_states_of_free_runs(backend):
    """linear_fast: the state after the last step, for the environments that never ended -- lanes exact, positions 1e-6."""
    g = TrafficGolden("linear_fast")
    eng = _engine(backend, g)
    eng.set_state(g.state("init"))
    eng.set_behavior(g.behavior)
    ended = np.zeros(g.E, bool)
    for t in range(g.steps):
        ended |= eng.step(g.actions_at(t))[2]
    got, want = eng.get_state(), g.state("step", g.steps - 1)
    eng.close()
    rows = ~ended
    for k in ("lane", "target_lane"):
        np.testing.assert_array_equal(got[k][rows], want[k][rows], err_msg=k)
    for k in ("x", "y", "speed"):
        np.testing.assert_allclose(got[k][rows], want[k][rows], rtol=0, atol=1e-6, err_msg=k)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", ["linear_fast", "linear_v0", "linear_n100"])
def test_rollout_k4_equals_four_steps(backend, name):
    g = TrafficGolden(name)
    K = 3 if g.steps < 4 else 4
    acts = np.stack([g.actions_at(t) for t in range(K)])
    a = _engine(backend, g)
    b = _engine(backend, g)
    for e in (a, b):
        e.set_state(g.state("init"))
        e.set_behavior(g.behavior)
    ro = a.rollout(acts)  # one multi-step launch of the workgroup kernel
    steps = [b.step(acts[k]) for k in range(K)]
    for k in range(K):
        for j in range(4):
            np.testing.assert_array_equal(ro[j][k], steps[k][j], err_msg=f"step {k} output {j}")
    sa, sb = a.get_state(), b.get_state()
    for key in _abi.STATE_F64 + _abi.STATE_I32:
        np.testing.assert_array_equal(sa[key], sb[key], err_msg=key)
    a.close()
    b.close()


def _linear_cfg(E, **over):
    d = _abi.highway_fast_default_config()
    d.update({"vehicles_count": 50, "lanes_count": 4, "other_vehicles_type": "highway_env.vehicle.behavior.LinearVehicle"})
    d.update(over)
    return d, _abi.make_config(d, E, fast=True)


@pytest.mark.parametrize("backend", BACKENDS)
def test_device_reset_draws_the_rule_on_philox_uniforms(backend):
    """hwy_reset with Linear traffic against the yardstick of tests/spawn_util.py (the Python Philox and the reference's rule, nothing
    compiled from the kernel source): the parameters are spawn.behavior_from_draws of the Philox uniforms 2 .. 4 of every vehicle, bit
    for bit; the kinematic planes are the rule on draws 0 and 1 (what an IDM reset draws), the first observation is the oracle's of
    that state.  Beside it, as before: the emulator's own Philox gives the same parameters (every draw of every vehicle), and every
    state plane is, bit for bit, what the emulated IDM reset spawns on the same seeds."""
    from tests import spawn_util
    from tests.emu import emu
    E = 8
    d, cfg = _linear_cfg(E)
    eng = make_engine(backend, cfg)
    seeds = np.arange(E, dtype=np.uint64) * 7919 + 3
    kw = dict(ego_spacing=d["ego_spacing"], vehicles_density=d["vehicles_density"])
    obs = eng.reset(seeds=seeds, **kw)
    got = eng.get_behavior()
    st = eng.get_state()
    want = spawn_util.assert_spawned(d, cfg, eng, np.arange(E), seeds, 0, obs, kw, "Linear reset")
    eng.close()
    np.testing.assert_array_equal(got, want["behavior"])
    assert (np.diff(want["x"], axis=1) > 0).all() and got[:, 1:].all()
    u = np.zeros((E, cfg.num_vehicles, 5))
    for e in range(E):
        for i in range(cfg.num_vehicles):
            a0, a1 = emu.philox_uniform2(int(seeds[e]), i, 0, 2)
            a2, s0 = emu.philox_uniform2(int(seeds[e]), i, 0, 3)
            s1, _ = emu.philox_uniform2(int(seeds[e]), i, 0, 4)
            u[e, i] = [a0, a1, a2, s0, s1]
            for draw in (0, 1):
                assert emu.philox_uniform2(int(seeds[e]), i, 0, draw) == spawn_util.philox_uniform2(int(seeds[e]), i, 0, draw)
    np.testing.assert_array_equal(got, spawn.behavior_from_draws(cfg, u))
    # the kinematic spawn is the IDM reset's
    from tests.emu.emu import EmuEngine
    idm = EmuEngine(_abi.make_config(dict(d, other_vehicles_type="highway_env.vehicle.behavior.IDMVehicle"), E, fast=True))
    idm.reset(seeds=seeds, **kw)
    ref = idm.get_state()
    idm.close()
    for k in _abi.STATE_F64 + _abi.STATE_I32:
        np.testing.assert_array_equal(st[k], ref[k], err_msg=k)


@pytest.mark.parametrize("backend", BACKENDS)
def test_autoreset_respawns_parameters(backend):
    """An environment that ends is re-spawned with episode + 1's state and parameters: the rule on the next Philox stream of its
    auto-reset seed, computed in Python (tests/spawn_util.py).  Beside it, the kernel's own draw function compiled for the CPU
    (emu.behavior_draw) gives the same parameters."""
    from tests import spawn_util
    E = 4
    d, cfg = _linear_cfg(E, vehicles_count=20, lanes_count=3, duration=2)
    eng = make_engine(backend, cfg)
    kw = dict(ego_spacing=d["ego_spacing"], vehicles_density=d["vehicles_density"])
    eng.reset(seeds=np.arange(E, dtype=np.uint64), **kw)
    eng.set_autoreset(True, base_seed=11, **kw)
    idle = np.ones((E, 1), np.int32)
    _, _, te, tr, _ = eng.step(idle)
    assert not (te | tr).any()
    _, _, te, tr, _ = eng.step(idle)
    assert (te | tr).all()  # duration 2 at policy frequency 1: every environment ends in its second step ...
    out = eng.step(idle)    # ... and is re-spawned in the third (next-step auto-reset: reward 0, not done)
    _, reward, te, tr, _ = out
    assert not (te | tr).any() and not reward.any()
    got = eng.get_behavior()
    spawn_util.assert_spawned(d, cfg, eng, np.arange(E), 11 + np.arange(E), 1, out, kw, "Linear re-spawn")
    eng.close()
    np.testing.assert_array_equal(got, spawn_util.expected_behavior(cfg, 11 + np.arange(E), 1))
    from tests.emu import emu
    for e in range(E):
        for i in range(1, cfg.num_vehicles):
            np.testing.assert_array_equal(got[e, i], emu.behavior_draw(11 + e, i, 1), err_msg=f"env {e} vehicle {i}")


def test_tan_bounded_within_2_ulp_emu():
    _check_tan("emu")


@pytest.mark.gpu
def test_tan_bounded_within_2_ulp_hip():
    _check_tan("hip")


def _check_tan(backend):
    """The steering's tan (hwy_math.h: tan_bounded, probe op 12) on |x| <= pi/3 against numpy's tan."""
    _, cfg = _linear_cfg(1)
    eng = make_engine(backend, cfg)
    x = np.concatenate([np.linspace(-np.pi / 3, np.pi / 3, 400001), np.random.default_rng(0).uniform(-np.pi / 3, np.pi / 3, 200000)])
    got = eng.debug_math(12, x)
    eng.close()
    want = np.tan(x)
    ulp = np.abs(got - want) / np.spacing(np.abs(want))
    assert ulp.max() <= 2.0, ulp.max()


@pytest.mark.gpu
def test_hip_equals_emu_on_random_configs():
    """E = 256 environments per configuration, random shapes, device reset and three steps: the engine against the emulation."""
    rng = np.random.default_rng(2024)
    for case in range(4):
        cls = ["LinearVehicle", "AggressiveVehicle", "DefensiveVehicle"][case % 3]
        d = (_abi.highway_fast_default_config() if case % 2 == 0 else _abi.highway_default_config())
        d.update({"vehicles_count": int(rng.integers(5, 120)), "lanes_count": int(rng.integers(2, 6)),
                  "vehicles_density": float(rng.uniform(0.8, 2.0)), "controlled_vehicles": int(rng.integers(1, 3)),
                  "other_vehicles_type": "highway_env.vehicle.behavior." + cls})
        cfg = _abi.make_config(d, 256, fast=case % 2 == 0)
        engines = [make_engine(b, cfg) for b in ("hip", "emu")]
        for eng in engines:
            eng.reset(seeds=np.arange(256, dtype=np.uint64) + 100 * case, ego_spacing=d["ego_spacing"],
                      vehicles_density=d["vehicles_density"])
        np.testing.assert_array_equal(engines[0].get_behavior(), engines[1].get_behavior())
        for t in range(3):
            acts = rng.integers(0, 5, size=(256, cfg.num_agents)).astype(np.int32)
            outs = [eng.step(acts) for eng in engines]
            np.testing.assert_allclose(outs[0][0], outs[1][0], rtol=0, atol=1e-6, err_msg=f"case {case} step {t}: obs")
            np.testing.assert_allclose(outs[0][1], outs[1][1], rtol=0, atol=1e-9)
            np.testing.assert_array_equal(outs[0][2], outs[1][2])
        s0, s1 = engines[0].get_state(), engines[1].get_state()
        np.testing.assert_array_equal(s0["lane"], s1["lane"])
        np.testing.assert_allclose(s0["x"], s1["x"], rtol=0, atol=1e-7)
        for eng in engines:
            eng.close()
