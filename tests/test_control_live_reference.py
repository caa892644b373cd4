"""The direct-ego-control kernels (CPU emulation, tests/emu/emu.py) against the LIVE unmodified reference on random
configurations: drawn over vehicles_count, lanes_count, vehicles_density, simulation / policy frequency, controlled_vehicles,
highway-v0 / highway-fast-v0 and the DiscreteAction keys (actions_per_axis, the two ranges, longitudinal / lateral, clip).  The
reference is driven by the fixture generator (tests/golden/control/make_golden_control.py: run) and the emulation is held to the
fixtures' checks: the axis tables and the host spawn bit for bit, then every policy step's observation at 1e-6, reward at 1e-9,
terminated / truncated / crashed and the lanes exact, the egos' speed and stored acceleration bit for bit, up to the first
termination.  Build container only (the reference does not exist on the GPU machines).  HWY_CONTROL_REF_CASES: configurations
(default 24)."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

from highwayenv_amd import spawn
from oracle import ref_stub
from tests.families_util import check_free_running_steps
from tests.control_util import CONTROL_DIR, ControlGolden, make_engine

pytestmark = [pytest.mark.reference,
              pytest.mark.skipif(not ref_stub.reference_available(), reason="needs the reference package")]

CASES = range(int(os.environ.get("HWY_CONTROL_REF_CASES", "24")))


def _generator():
    mgc = sys.modules.get("make_golden_control")
    if mgc is None:
        spec = importlib.util.spec_from_file_location("make_golden_control", os.path.join(CONTROL_DIR, "make_golden_control.py"))
        mgc = importlib.util.module_from_spec(spec)
        sys.modules["make_golden_control"] = mgc
        spec.loader.exec_module(mgc)
    return mgc


def _draw(case: int) -> dict:
    mgc = _generator()
    rng = np.random.default_rng(88_000 + case)
    fast = bool(rng.integers(0, 2))
    A = int(rng.choice([1, 1, 2]))
    steer = float(np.round(rng.choice([0.03, 0.08, 0.2, np.pi / 4]), 4))
    lo, hi = float(np.round(rng.uniform(-6, -1), 2)), float(np.round(rng.uniform(1, 6), 2))
    axes = int(rng.choice([0, 0, 0, 1, 2]))  # both / longitudinal only / lateral only
    act = mgc.discrete(actions_per_axis=int(rng.integers(2, 7)), steering_range=[-steer, steer], acceleration_range=[lo, hi],
                       longitudinal=axes != 2, lateral=axes != 1, clip=bool(rng.integers(0, 2)))
    config = {"vehicles_count": int(rng.integers(5, 46)), "lanes_count": int(rng.integers(2, 6)),
              "vehicles_density": float(np.round(rng.uniform(0.7, 2.2), 3)), "simulation_frequency": int(rng.choice([5, 10, 15])),
              "policy_frequency": int(rng.choice([1, 2])), "ego_spacing": float(np.round(rng.uniform(1.0, 2.5), 3)),
              "duration": 20, "offroad_terminal": bool(rng.integers(0, 2)), "action": act}
    if A > 1:
        config.update({"controlled_vehicles": A, "action": {"type": "MultiAgentAction", "action_config": act},
                       "observation": {"type": "MultiAgentObservation", "observation_config": {"type": "Kinematics"}}})
    return dict(name=f"live_direct_{case}", cls=mgc.HighwayEnvFast if fast else mgc.HighwayEnv, config=config,
                seeds=[int(rng.integers(0, 2**31))], steps=6, action_seed=int(rng.integers(0, 2**31)), frames_for=0)


@pytest.mark.parametrize("case", CASES)
def test_emulation_against_live_reference(case):
    sc = _draw(case)
    data = _generator().run(sc)
    g = ControlGolden(sc["name"], data)
    cfg = g.hwy_config()
    n = cfg.n_accel * cfg.n_steer
    np.testing.assert_array_equal([cfg.accel_axis[a // cfg.n_steer] for a in range(n)], g.z["axis_accel"])
    np.testing.assert_array_equal([cfg.steer_axis[a % cfg.n_steer] for a in range(n)], g.z["axis_steer"])
    st = spawn.spawn_reference_stream(cfg, g.seeds, g.config["ego_spacing"], g.config["vehicles_density"])
    want0 = g.state("init")
    for k in ("x", "y", "speed", "lane", "flags"):
        np.testing.assert_array_equal(st[k], want0[k], err_msg=f"{sc['name']}: spawn {k}")
    eng = make_engine("emu", cfg)
    eng.set_state(st)  # (the host spawn's own state: the ego's target-speed slot is not what the kernels read)
    z = g.z
    agents = list(cfg.agent_index[:g.A])
    for t in range(g.steps):
        obs, reward, term, trunc, info = eng.step(g.actions_at(t))
        what = f"{sc['name']} ({json.dumps(sc['config'])}) step {t}"
        np.testing.assert_allclose(obs, z["obs"][t].reshape(obs.shape), rtol=0, atol=1e-6, err_msg=what + ": obs")
        np.testing.assert_allclose(reward[:, 0], z["reward"][t], rtol=0, atol=1e-9, err_msg=what + ": reward")
        np.testing.assert_array_equal(term, z["terminated"][t].astype(bool), err_msg=what + ": terminated")
        np.testing.assert_array_equal(trunc, z["truncated"][t].astype(bool), err_msg=what + ": truncated")
        np.testing.assert_array_equal(info["crashed"], z["step_crashed"][t][:, agents] != 0, err_msg=what + ": crashed")
        got = eng.get_state()
        for k in ("lane", "target_lane"):
            np.testing.assert_array_equal(got[k], z["step_" + k][t], err_msg=what + ": " + k)
        np.testing.assert_array_equal(got["speed"][:, agents], z["step_speed"][t][:, agents], err_msg=what + ": the egos' speed")
        np.testing.assert_array_equal(eng.get_controls()[0], z["step_act_accel"][t][:, agents], err_msg=what + ": stored acceleration")
        if term[0]:
            break
    check_free_running_steps(g)  # the same run through the oracle: state 1e-8, the egos' speed and stored action bit for bit
