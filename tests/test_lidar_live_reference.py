"""The LidarObservation kernel (CPU emulation, tests/emu/emu.py) against the LIVE unmodified reference on random
configurations: drawn over cells, maximum_range, normalize, vehicles_count, lanes_count, vehicles_density, the frequencies,
controlled_vehicles, highway-v0 / highway-fast-v0 and the family (IDM traffic, LinearVehicle traffic, DiscreteAction ego).  The
reference is driven by the fixture generator (tests/golden/lidar/make_golden_lidar.py: run).  Every recorded state is loaded and
observed, and the episode is run freely from the initial state up to the first termination: no cell differs beyond 1e-6.  Build
container only (the reference does not exist on the GPU machines).  The list of cases is fixed: seeds 0 .. 23 of `_draw`."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

from oracle import ref_stub
from oracle import oracle
from tests.families_util import check_free_running_steps, golden_state
from tests.lidar_util import LIDAR_DIR, OBS_ATOL, LidarGolden, cells_off, make_engine

pytestmark = [pytest.mark.reference,
              pytest.mark.skipif(not ref_stub.reference_available(), reason="needs the reference package")]

CASES = range(24)


def _generator():
    mgl = sys.modules.get("make_golden_lidar")
    if mgl is None:
        spec = importlib.util.spec_from_file_location("make_golden_lidar", os.path.join(LIDAR_DIR, "make_golden_lidar.py"))
        mgl = importlib.util.module_from_spec(spec)
        sys.modules["make_golden_lidar"] = mgl
        spec.loader.exec_module(mgl)
    return mgl


def _draw(case: int) -> dict:
    mgl = _generator()
    rng = np.random.default_rng(91_000 + case)
    fast = bool(rng.integers(0, 2))
    family = ["idm", "idm", "linear", "direct"][int(rng.integers(0, 4))]
    A = int(rng.choice([1, 1, 2])) if family != "linear" else 1
    obs = mgl.lidar(cells=int(rng.choice([1, 2, 3, 7, 8, 16, 16, 24, 36, 63, 64])), maximum_range=float(np.round(rng.uniform(15, 150), 2)),
                    normalize=bool(rng.integers(0, 2)))
    config = {"vehicles_count": int(rng.integers(3, 80)), "lanes_count": int(rng.integers(1, 6)),
              "vehicles_density": float(np.round(rng.uniform(0.7, 2.5), 3)), "simulation_frequency": int(rng.choice([5, 10, 15])),
              "policy_frequency": int(rng.choice([1, 2])), "ego_spacing": float(np.round(rng.uniform(1.0, 2.5), 3)),
              "duration": 20, "observation": obs}
    act = {"type": "DiscreteAction", "steering_range": [-0.2, 0.2]} if family == "direct" else {"type": "DiscreteMetaAction"}
    if family == "linear":
        config["other_vehicles_type"] = mgl.LINEAR
    config["action"] = act
    if A > 1:
        config.update({"controlled_vehicles": A, "action": {"type": "MultiAgentAction", "action_config": act},
                       "observation": {"type": "MultiAgentObservation", "observation_config": obs}})
    return dict(name=f"live_lidar_{case}", cls=mgl.HighwayEnvFast if fast else mgl.HighwayEnv, config=config,
                seeds=[int(rng.integers(0, 2**31))], steps=5, action_seed=int(rng.integers(0, 2**31)))


@pytest.mark.parametrize("case", CASES)
def test_emulation_against_live_reference(case):
    sc = _draw(case)
    g = LidarGolden(sc["name"], _generator().run(sc))
    what = f"{sc['name']} ({json.dumps(sc['config'])})"
    eng = make_engine("emu", g.hwy_config())
    off = total = 0
    for index in [None] + list(range(g.steps)):
        g.load(eng, "init" if index is None else "step", index)
        got, want = eng.observe(), g.reference_obs(index)
        off += cells_off(got, want)
        total += want[..., 0].size
    assert off == 0, f"{what}: {off} of {total} cells of the recorded states differ beyond {OBS_ATOL}"
    g.load(eng)
    alive = np.ones(g.E, bool)
    for t in range(g.steps):
        obs, reward, term, trunc, info = eng.step(g.actions_at(t))
        rows = np.flatnonzero(alive)
        assert cells_off(obs[rows], g.reference_obs(t)[rows]) == 0, f"{what}: free running, step {t}"
        np.testing.assert_array_equal(term[rows], g.z["terminated"][t][rows].astype(bool), err_msg=f"{what} step {t}: terminated")
        alive &= ~np.asarray(term, bool)
    eng.close()
    # the same case through the oracle: every recorded state traced, then the free run (no cell beyond 1e-6 in either)
    cfg = g.hwy_config()
    for index in [None] + list(range(g.steps)):
        st = golden_state(g, "init" if index is None else "step", index)
        assert cells_off(oracle.observe(cfg, st), g.reference_obs(index)) == 0, f"{what}: the oracle on recorded state {index}"
    check_free_running_steps(g)
