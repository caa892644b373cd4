"""Direct ego control (the reference's ``DiscreteAction``: the DirectEgo policy of the one-wavefront kernel, hwy_wave.h:
hwy_step_wave_direct_kernel / hwy_rollout_wave_direct_kernel for N <= 64, and of the workgroup kernel, hwy_device.h:
hwy_step_direct_kernel / hwy_rollout_direct_kernel / hwy_reset_direct_kernel) against the unmodified reference's fixtures
(tests/golden/control), on the CPU emulation of the kernel source (``emu``) and on the MI355X (``hip``).

Here the reference's own traces are the yardstick; the C oracle restates the plain-Vehicle ego too (pinned to these fixtures by
tests/test_oracle_golden_families.py) and is the yardstick beyond their shapes (tests/test_fuzz_configs.py, tests/test_families_edge_cases.py).  The ego's speed is a closed recurrence on
exactly rounded operations (speed += a * dt as a product and a sum, MAX_SPEED - speed, -1.0 * speed), so it and the stored
acceleration are compared BIT FOR BIT; a teacher-forced frame whose discrete outcome differs from the reference's would be a knife
edge, and the budget for those is 0 on every fixture."""
import numpy as np
import pytest

from highwayenv_amd import _abi
from tests import spawn_util
from tests.control_util import BACKENDS, FIXTURES, WITH_FRAMES, ControlGolden, make_engine
from tests.golden_util import assert_state_close

KNIFE_FRAMES = {name: 0 for name in FIXTURES}


def _engine(backend, g: ControlGolden, envs=None, tuning=None):
    return make_engine(backend, g.hwy_config(len(envs) if envs is not None else None, tuning=tuning))


def _start(eng, g: ControlGolden):
    eng.set_state(g.state("init"))
    eng.set_controls(*g.controls("init"))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", WITH_FRAMES)
def test_teacher_forced_frames(backend, name):
    """Every recorded frame from the reference's own previous frame (state AND stored controls): positions and headings at 1e-9,
    the ego's speed and its stored acceleration and steering bit-identical, lanes and flags exact."""
    g = ControlGolden(name)
    envs = list(range(g.frames_for))
    eng = _engine(backend, g, envs)
    agents = list(g.hwy_config().agent_index[:g.A])
    edges = 0
    for j in range(g.steps * g.T):
        t, f = divmod(j, g.T)
        where = ("init", None) if j == 0 else ("frame", j - 1)
        eng.set_state(g.state(*where, envs=envs))
        eng.set_controls(*g.controls(*where, envs=envs))
        eng.step_frames(g.actions_at(t)[envs] if f == 0 else None, 1)
        got, want = eng.get_state(), g.state("frame", j, envs=envs)
        if not all(np.array_equal(got[k], want[k]) for k in ("lane", "target_lane", "flags")):
            edges += 1
            continue
        assert_state_close(got, want, atol=1e-9, what=f"{name} frame {j}")
        np.testing.assert_array_equal(got["speed"][:, agents], want["speed"][:, agents], err_msg=f"{name} frame {j}: the ego's speed")
        accel, steer = eng.get_controls()
        want_accel, want_steer = g.controls("frame", j, envs=envs)
        np.testing.assert_array_equal(accel, want_accel, err_msg=f"{name} frame {j}: stored acceleration")
        np.testing.assert_array_equal(steer, want_steer, err_msg=f"{name} frame {j}: stored steering")
    eng.close()
    assert edges <= KNIFE_FRAMES[name], f"{name}: {edges} knife-edge frames"


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", FIXTURES)
def test_free_running_episodes(backend, name):
    """Whole episodes from the reference's initial state: obs 1e-6, reward 1e-9, crashed / terminated / truncated and lanes exact,
    each environment up to and including its first terminated step (afterwards the reference keeps stepping a finished one)."""
    g = ControlGolden(name)
    eng = _engine(backend, g)
    _start(eng, g)
    z = g.z
    agents = list(g.hwy_config().agent_index[:g.A])
    alive = np.ones(g.E, bool)
    for t in range(g.steps):
        obs, reward, term, trunc, info = eng.step(g.actions_at(t))
        got = eng.get_state()
        rows = np.flatnonzero(alive)
        for k in ("lane", "target_lane"):
            np.testing.assert_array_equal(got[k][rows], z["step_" + k][t][rows], err_msg=f"{name} step {t}: {k}")
        np.testing.assert_allclose(obs[rows], z["obs"][t].reshape(obs.shape)[rows], rtol=0, atol=1e-6, err_msg=f"{name} step {t}: obs")
        np.testing.assert_allclose(reward[rows, 0], z["reward"][t][rows], rtol=0, atol=1e-9, err_msg=f"{name} step {t}: reward")
        np.testing.assert_array_equal(term[rows], z["terminated"][t][rows].astype(bool), err_msg=f"{name} step {t}: terminated")
        np.testing.assert_array_equal(trunc[rows], z["truncated"][t][rows].astype(bool), err_msg=f"{name} step {t}: truncated")
        np.testing.assert_array_equal(info["crashed"][rows], z["step_crashed"][t][rows][:, agents] != 0, err_msg=f"{name} step {t}: crashed")
        alive &= ~np.asarray(term, bool)
    eng.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_brake_run_ends_on_the_reference_speed_bit_for_bit(backend):
    """direct_brake, free running for all 20 steps (300 frames through speed 0, off the road start and into the MIN_SPEED clip): the
    ego's speed after every step is the reference's double -- a fused speed update takes the other branch of the clip here."""
    g = ControlGolden("direct_brake")
    eng = _engine(backend, g)
    _start(eng, g)
    ego = g.hwy_config().agent_index[0]
    assert not g.z["terminated"].any()
    for t in range(g.steps):
        eng.step(g.actions_at(t))
        np.testing.assert_array_equal(eng.get_state()["speed"][:, ego], g.z["step_speed"][t][:, ego], err_msg=f"step {t}")
        np.testing.assert_array_equal(eng.get_controls()[0][:, 0], g.z["step_act_accel"][t][:, ego], err_msg=f"step {t}: stored acceleration")
    eng.close()
    assert g.z["step_speed"][-1][:, ego].min() < -40.0 and (g.z["step_x"][-1][:, ego] < 0).all()  # (what the fixture is for)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", [n for n in FIXTURES if n != "direct_n100"])
def test_wave_and_workgroup_kernels_bit_identical(backend, name):
    """N <= 64: the one-wavefront kernel (the engine's choice) and the workgroup kernel (tune_block_kernel = 1) give the same
    simulation, bit for bit, over the whole fixture: every state plane, the stored controls, reward, terminated / truncated /
    crashed.  The f32 observation may be one f32 rounding apart (the one-wavefront kernel's observe multiplies by host-computed
    reciprocals of the feature ranges): 1e-6."""
    g = ControlGolden(name)
    engines = [_engine(backend, g, tuning={"block_kernel": b}) for b in (0, 1)]
    for eng in engines:
        _start(eng, g)
    for t in range(g.steps):
        outs = [eng.step(g.actions_at(t)) for eng in engines]
        np.testing.assert_allclose(outs[0][0], outs[1][0], rtol=0, atol=1e-6, err_msg=f"{name} step {t}: obs")
        for j in (1, 2, 3):
            np.testing.assert_array_equal(outs[0][j], outs[1][j], err_msg=f"{name} step {t} output {j}")
        np.testing.assert_array_equal(outs[0][4]["crashed"], outs[1][4]["crashed"])
    sa, sb = engines[0].get_state(), engines[1].get_state()
    for key in _abi.STATE_F64 + _abi.STATE_I32:
        np.testing.assert_array_equal(sa[key], sb[key], err_msg=key)
    for a, b in zip(engines[0].get_controls(), engines[1].get_controls()):
        np.testing.assert_array_equal(a, b)
    for eng in engines:
        eng.close()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", ["direct_fast", "direct_v0", "direct_throttle", "direct_ma2", "direct_n100"])
def test_rollout_equals_steps(backend, name):
    """hwy_rollout (K steps in one launch) equals K calls of hwy_step, bit for bit: outputs, state and stored controls."""
    g = ControlGolden(name)
    K = min(g.steps, 4)
    acts = np.stack([g.actions_at(t) for t in range(K)])
    a, b = _engine(backend, g), _engine(backend, g)
    for e in (a, b):
        _start(e, g)
    ro = a.rollout(acts)
    steps = [b.step(acts[k]) for k in range(K)]
    for k in range(K):
        for j in range(4):
            np.testing.assert_array_equal(ro[j][k], steps[k][j], err_msg=f"step {k} output {j}")
    sa, sb = a.get_state(), b.get_state()
    for key in _abi.STATE_F64 + _abi.STATE_I32:
        np.testing.assert_array_equal(sa[key], sb[key], err_msg=key)
    for x, y in zip(a.get_controls(), b.get_controls()):
        np.testing.assert_array_equal(x, y)
    a.close()
    b.close()


def _direct_cfg(E, fast=True, **over):
    d = _abi.highway_fast_default_config() if fast else _abi.highway_default_config()
    d.update({"vehicles_count": 50, "lanes_count": 4, "action": {"type": "DiscreteAction", "steering_range": [-0.05, 0.05]}})
    d.update(over)
    return d, _abi.make_config(d, E, fast=fast)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n", [50, 100])
def test_device_reset_is_the_meta_action_reset_with_zero_controls(backend, n):
    """hwy_reset of a direct-control engine against the yardstick of tests/spawn_util.py (the Python Philox and the reference's rule,
    nothing compiled from the kernel source): every state plane, the first observation and zero stored controls.  Beside it: every
    plane is bit for bit the one the emulated meta-action engine's reset writes for the same seeds (same Philox draws)."""
    from tests.emu.emu import EmuEngine
    E = 8
    d, cfg = _direct_cfg(E, vehicles_count=n)
    eng = make_engine(backend, cfg)
    eng.set_controls(np.full((E, 1), 3.0), np.full((E, 1), 0.25))
    seeds = np.arange(E, dtype=np.uint64) * 7919 + 3
    kw = dict(ego_spacing=d["ego_spacing"], vehicles_density=d["vehicles_density"])
    obs = eng.reset(seeds=seeds, **kw)
    st = eng.get_state()
    accel, steer = eng.get_controls()
    spawn_util.assert_spawned(d, cfg, eng, np.arange(E), seeds, 0, obs, kw, "direct-control reset")
    eng.close()
    assert not accel.any() and not steer.any()
    meta = EmuEngine(_abi.make_config(dict(d, action={"type": "DiscreteMetaAction"}), E, fast=True))
    obs_meta = meta.reset(seeds=seeds, **kw)
    ref = meta.get_state()
    for k in _abi.STATE_F64 + _abi.STATE_I32:
        np.testing.assert_array_equal(st[k], ref[k], err_msg=k)
    np.testing.assert_array_equal(obs, obs_meta)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("block_kernel", [0, 1])
def test_autoreset_clears_the_controls(backend, block_kernel):
    """An environment that ends is re-spawned in the next step with zero stored controls (Vehicle.__init__), whatever it held."""
    E = 4
    d, _ = _direct_cfg(E, vehicles_count=20, lanes_count=3, duration=2)
    cfg = _abi.make_config(d, E, fast=True, tuning={"block_kernel": block_kernel})
    eng = make_engine(backend, cfg)
    eng.reset(seeds=np.arange(E, dtype=np.uint64), ego_spacing=d["ego_spacing"], vehicles_density=d["vehicles_density"])
    eng.set_autoreset(True, base_seed=11, ego_spacing=d["ego_spacing"], vehicles_density=d["vehicles_density"])
    gas = np.full((E, 1), 8, np.int32)  # full throttle, steering right
    _, _, te, tr, _ = eng.step(gas)
    assert not (te | tr).any()
    accel, steer = eng.get_controls()
    assert (accel == 5.0).all() and (steer == cfg.steer_axis[2]).all()
    _, _, te, tr, _ = eng.step(gas)
    assert (te | tr).all()  # duration 2 at policy frequency 1: every environment ends in its second step ...
    out = eng.step(gas)  # ... and is re-spawned in the third (next-step auto-reset: reward 0, not done)
    _, reward, te, tr, _ = out
    assert not (te | tr).any() and not reward.any()
    accel, steer = eng.get_controls()
    # (the whole re-spawn against the rule on the Python Philox: state, observation, outputs, zero controls)
    kw = dict(ego_spacing=d["ego_spacing"], vehicles_density=d["vehicles_density"])
    spawn_util.assert_spawned(d, cfg, eng, np.arange(E), 11 + np.arange(E), 1, out, kw, "direct-control re-spawn")
    eng.close()
    assert not accel.any() and not steer.any()


@pytest.mark.parametrize("backend", BACKENDS)
def test_frames_without_an_action_continue_with_the_stored_controls(backend):
    """hwy_step_frames(actions = NULL) is Vehicle.act(None): the stored pair drives on.  direct_throttle, step 2 in two halves."""
    g = ControlGolden("direct_throttle")
    envs = list(range(g.frames_for))
    a, b = _engine(backend, g, envs), _engine(backend, g, envs)
    for e in (a, b):
        e.set_state(g.state("step", 1, envs=envs))
        e.set_controls(*g.controls("step", 1, envs=envs))
    a.step_frames(g.actions_at(2)[envs], g.T)
    b.step_frames(g.actions_at(2)[envs], 2)
    b.step_frames(None, g.T - 2)
    sa, sb = a.get_state(), b.get_state()
    for key in _abi.STATE_F64 + _abi.STATE_I32:
        np.testing.assert_array_equal(sa[key], sb[key], err_msg=key)
    np.testing.assert_array_equal(a.get_controls()[0], b.get_controls()[0])
    np.testing.assert_array_equal(a.get_controls()[0], g.controls("step", 2, envs=envs)[0])
    a.close()
    b.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_ids_outside_the_table_raise_index_error(backend):
    _, cfg = _direct_cfg(2)
    eng = make_engine(backend, cfg)
    eng.reset(seeds=np.arange(2, dtype=np.uint64))
    for bad in (9, -1):  # (the reference's list lookup would wrap -1: rejected here, hwy_engine.h)
        with pytest.raises(IndexError):
            eng.step(np.array([[0], [bad]], np.int32))
    eng.close()


@pytest.mark.gpu
def test_hip_equals_emu_on_random_configs():
    """E = 256 environments per configuration, random shapes and action tables, device reset and three steps: the engine against
    the emulation."""
    rng = np.random.default_rng(2025)
    for case in range(4):
        fast = case % 2 == 0
        act = {"type": "DiscreteAction", "actions_per_axis": int(rng.integers(2, 6)),
               "steering_range": [-float(rng.uniform(0.02, 0.3))] * 2, "longitudinal": case != 1, "lateral": case != 3}
        act["steering_range"][1] = -act["steering_range"][0]
        A = int(rng.integers(1, 3))
        d, _ = _direct_cfg(256, fast=fast, vehicles_count=int(rng.integers(5, 120)), lanes_count=int(rng.integers(2, 6)),
                           vehicles_density=float(rng.uniform(0.8, 2.0)), controlled_vehicles=A,
                           action=act if A == 1 else {"type": "MultiAgentAction", "action_config": act})
        cfg = _abi.make_config(d, 256, fast=fast)
        engines = [make_engine(b, cfg) for b in ("hip", "emu")]
        for eng in engines:
            eng.reset(seeds=np.arange(256, dtype=np.uint64) + 100 * case, ego_spacing=d["ego_spacing"],
                      vehicles_density=d["vehicles_density"])
        for t in range(3):
            acts = rng.integers(0, _abi.num_actions(cfg), size=(256, cfg.num_agents)).astype(np.int32)
            outs = [eng.step(acts) for eng in engines]
            np.testing.assert_allclose(outs[0][0], outs[1][0], rtol=0, atol=1e-6, err_msg=f"case {case} step {t}: obs")
            np.testing.assert_allclose(outs[0][1], outs[1][1], rtol=0, atol=1e-9)
            np.testing.assert_array_equal(outs[0][2], outs[1][2])
        s0, s1 = engines[0].get_state(), engines[1].get_state()
        np.testing.assert_array_equal(s0["lane"], s1["lane"])
        np.testing.assert_allclose(s0["x"], s1["x"], rtol=0, atol=1e-7)
        agents = list(cfg.agent_index[:cfg.num_agents])
        np.testing.assert_array_equal(s0["speed"][:, agents], s1["speed"][:, agents])  # the egos' speed: exactly rounded operations
        for x, y in zip(engines[0].get_controls(), engines[1].get_controls()):
            np.testing.assert_array_equal(x, y)
        for eng in engines:
            eng.close()
