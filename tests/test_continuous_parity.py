"""Continuous control (csrc/hwy_act.h in front of the direct-control step kernels) against fixtures of the unmodified reference run
with ``{"type": "ContinuousAction", ...}`` (tests/golden/continuous), on the CPU emulation of the kernel source (``emu``) and on
the MI355X (``hip``).  The engine is configured with the matching ``DiscreteAction`` dict and driven through ``step_continuous``.

Tolerances and knife-edge exclusions are those of tests/test_control_parity.py: positions and headings of a teacher-forced frame
at 1e-9, the ego's speed and its stored pair bit for bit, lanes and flags exact with a budget of 0 knife-edge frames on every
fixture; free-running episodes at obs 1e-6, reward 1e-9, flags and lanes exact, each environment up to and including its first
terminated step."""
import hashlib
import json
import os

import numpy as np
import pytest

from highwayenv_amd import _abi
from tests.continuous_util import BACKENDS, CONTINUOUS_DIR, FIXTURES, ContinuousGolden, assert_states_equal, make_engine, restate
from tests.golden_util import assert_state_close

WITH_FRAMES = [n for n in FIXTURES if n != "cont_dense"]
KNIFE_FRAMES = {name: 0 for name in FIXTURES}


def _engine(backend, g: ContinuousGolden, envs=None, tuning=None):
    return make_engine(backend, g.hwy_config(len(envs) if envs is not None else None, tuning=tuning))


def _start(eng, g: ContinuousGolden):
    eng.set_state(g.state("init"))
    eng.set_controls(*g.controls("init"))


def _agents(g):
    return list(g.hwy_config().agent_index[:g.A])


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_is_the_committed_one_and_says_what_it_should(name):
    """Every fixture to its digest in tests/golden/continuous/MANIFEST.json; the reference ran a ContinuousAction on float32 actions
    beyond the clip, and its own mapped pairs are the restatement's (tests/continuous_util.py), bit for bit."""
    manifest = json.load(open(os.path.join(CONTINUOUS_DIR, "MANIFEST.json")))
    g = ContinuousGolden(name)
    h = hashlib.sha256()
    for k in sorted(g.z.files):
        a = np.asarray(g.z[k])
        h.update(k.encode())
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(np.ascontiguousarray(a).tobytes())
    assert h.hexdigest() == manifest[name]
    act = g.ref_action["action_config"] if g.ref_action["type"] == "MultiAgentAction" else g.ref_action
    assert act["type"] == "ContinuousAction" and g.z["actions"].dtype == np.float32
    assert np.abs(g.z["actions"]).max() > 1.0
    accel, steer = restate(g.params, g.z["actions"])
    np.testing.assert_array_equal(accel.view(np.uint64), g.z["mapped_accel"].view(np.uint64))
    np.testing.assert_array_equal(steer.view(np.uint64), g.z["mapped_steer"].view(np.uint64))


def test_fixtures_cover_what_they_are_for():
    z = {n: ContinuousGolden(n) for n in FIXTURES}
    assert z["cont_fast"].fast and not z["cont_v0"].fast and z["cont_v0"].T == 15
    assert [float(v) for v in z["cont_asym"].params.acceleration_range] == [-3.3, 2.1]
    assert [float(v) for v in z["cont_asym"].params.steering_range] == [-0.3, 0.1]
    assert all(float(np.float32(v)) != v for v in (-3.3, 2.1, -0.3, 0.1))
    assert z["cont_longi_only"].params.size == 1 and not z["cont_longi_only"].params.lateral
    assert z["cont_lat_only"].params.size == 1 and not z["cont_lat_only"].params.longitudinal
    assert z["cont_ma2"].A == 2 and z["cont_n100"].N == 101
    t = z["cont_throttle"]
    ego = t.hwy_config().agent_index[0]
    assert t.z["step_speed"][:, :, ego].max() > 40.0 and t.z["step_crashed"][-1][:, ego].any()  # the MAX_SPEED clip and a crash
    assert z["cont_dense"].z["terminated"].any(0).sum() >= 6


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", WITH_FRAMES)
def test_teacher_forced_frames(backend, name):
    """Every recorded frame from the reference's own previous frame (state AND stored controls); the first frame of a step behind
    the act launch on the reference's float32 action.  Right after that launch the stored pair is the reference's mapped pair
    bit for bit; after the frame it is the recorded one (where ``clip_actions`` rewrote it: the rewritten one)."""
    g = ContinuousGolden(name)
    envs = list(range(g.frames_for))
    eng = _engine(backend, g, envs)
    agents = _agents(g)
    edges = 0
    for j in range(g.steps * g.T):
        t, f = divmod(j, g.T)
        where = ("init", None) if j == 0 else ("frame", j - 1)
        eng.set_state(g.state(*where, envs=envs))
        eng.set_controls(*g.controls(*where, envs=envs))
        if f == 0:
            eng.act_continuous(g.params, g.actions_at(t)[envs])
            accel, steer = eng.get_controls()
            np.testing.assert_array_equal(accel, g.z["mapped_accel"][t][envs], err_msg=f"{name} step {t}: acceleration after the act launch")
            np.testing.assert_array_equal(steer, g.z["mapped_steer"][t][envs], err_msg=f"{name} step {t}: steering after the act launch")
        eng.step_frames(None, 1)
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
    """Whole episodes from the reference's initial state through ``step_continuous``.  Before every step the act launch alone, on a
    twin engine in the same state: its stored pair equals the fixture's recorded ``act_accel`` / ``act_steering`` bit for bit on
    every (step, environment, agent) where ``clip_actions`` did not rewrite it within the step -- most of them, on every fixture."""
    g = ContinuousGolden(name)
    eng, twin = _engine(backend, g), _engine(backend, g)
    _start(eng, g)
    z = g.z
    agents = _agents(g)
    alive = np.ones(g.E, bool)
    kept = total = 0
    for t in range(g.steps):
        twin.set_controls(*eng.get_controls())
        twin.act_continuous(g.params, g.actions_at(t))
        accel, steer = twin.get_controls()
        rec_accel, rec_steer = g.controls("step", t)
        same = (rec_accel == z["mapped_accel"][t]) & (rec_steer == z["mapped_steer"][t])  # clip_actions left the pair alone
        np.testing.assert_array_equal(accel[same], rec_accel[same], err_msg=f"{name} step {t}: acceleration after the act launch")
        np.testing.assert_array_equal(steer[same], rec_steer[same], err_msg=f"{name} step {t}: steering after the act launch")
        kept, total = kept + int(same.sum()), total + same.size
        obs, reward, term, trunc, info = eng.step_continuous(g.params, g.actions_at(t))
        got = eng.get_state()
        rows = np.flatnonzero(alive)
        for k in ("lane", "target_lane"):
            np.testing.assert_array_equal(got[k][rows], z["step_" + k][t][rows], err_msg=f"{name} step {t}: {k}")
        np.testing.assert_allclose(obs[rows], z["obs"][t].reshape(obs.shape)[rows], rtol=0, atol=1e-6, err_msg=f"{name} step {t}: obs")
        np.testing.assert_allclose(reward[rows, 0], z["reward"][t][rows], rtol=0, atol=1e-9, err_msg=f"{name} step {t}: reward")
        np.testing.assert_array_equal(term[rows], z["terminated"][t][rows].astype(bool), err_msg=f"{name} step {t}: terminated")
        np.testing.assert_array_equal(trunc[rows], z["truncated"][t][rows].astype(bool), err_msg=f"{name} step {t}: truncated")
        np.testing.assert_array_equal(info["crashed"][rows], z["step_crashed"][t][rows][:, agents] != 0, err_msg=f"{name} step {t}: crashed")
        # the stored pair after the step: the reference's, bit for bit (what clip_actions rewrote included)
        accel, steer = eng.get_controls()
        np.testing.assert_array_equal(accel[rows], rec_accel[rows], err_msg=f"{name} step {t}: stored acceleration")
        np.testing.assert_array_equal(steer[rows], rec_steer[rows], err_msg=f"{name} step {t}: stored steering")
        np.testing.assert_array_equal(got["speed"][rows][:, agents], z["step_speed"][t][rows][:, agents], err_msg=f"{name} step {t}: the ego's speed")
        alive &= ~np.asarray(term, bool)
    eng.close()
    twin.close()
    assert 2 * kept > total or name == "cont_throttle", (kept, total)  # (cont_throttle is in the clip for most of its run)
    assert kept >= 6  # (cont_n100 has 2 environments x 3 steps)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", ["cont_fast", "cont_ma2", "cont_throttle"])
def test_wave_and_workgroup_kernels_bit_identical(backend, name):
    """N <= 64: behind the same act launch the one-wavefront kernel and the workgroup kernel (tune_block_kernel = 1) give the same
    simulation, bit for bit (the f32 observation at 1e-6, as in tests/test_control_parity.py)."""
    g = ContinuousGolden(name)
    engines = [_engine(backend, g, tuning={"block_kernel": b}) for b in (0, 1)]
    for eng in engines:
        _start(eng, g)
    for t in range(g.steps):
        outs = [eng.step_continuous(g.params, g.actions_at(t)) for eng in engines]
        np.testing.assert_allclose(outs[0][0], outs[1][0], rtol=0, atol=1e-6, err_msg=f"{name} step {t}: obs")
        for j in (1, 2, 3):
            np.testing.assert_array_equal(outs[0][j], outs[1][j], err_msg=f"{name} step {t} output {j}")
    assert_states_equal(engines[0].get_state(), engines[1].get_state())
    for a, b in zip(engines[0].get_controls(), engines[1].get_controls()):
        np.testing.assert_array_equal(a, b)
    for eng in engines:
        eng.close()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", ["cont_throttle", "cont_ma2", "cont_n100"])
def test_rollout_equals_steps(backend, name):
    """``rollout_continuous`` with K = 4 (one call: four (act, step) launch pairs) equals four ``step_continuous`` calls, bit for
    bit: outputs, state and stored controls.  With next-step auto-reset on and, in cont_throttle, episodes that end inside."""
    g = ContinuousGolden(name)
    K = min(g.steps, 4)
    first = g.steps - K if name == "cont_throttle" else 0  # (its crashes are in the last steps)
    acts = np.stack([g.actions_at(first + k) for k in range(K)])
    a, b = _engine(backend, g), _engine(backend, g)
    for e in (a, b):
        where = ("init", None) if first == 0 else ("step", first - 1)
        e.set_state(g.state(*where))
        e.set_controls(*g.controls(*where))
        e.set_autoreset(True, base_seed=5, ego_spacing=g.config["ego_spacing"], vehicles_density=g.config["vehicles_density"])
    ro = a.rollout_continuous(g.params, acts)
    steps = [b.step_continuous(g.params, acts[k]) for k in range(K)]
    for k in range(K):
        for j in range(4):
            np.testing.assert_array_equal(ro[j][k], steps[k][j], err_msg=f"step {k} output {j}")
        for key in ("speed", "crashed"):
            np.testing.assert_array_equal(ro[4][key][k], steps[k][4][key])
    if name == "cont_throttle":
        done = ro[2] | ro[3]
        assert done[:-1].any(), "no episode ends inside the rollout"
    assert_states_equal(a.get_state(), b.get_state())
    for x, y in zip(a.get_controls(), b.get_controls()):
        np.testing.assert_array_equal(x, y)
    a.close()
    b.close()
