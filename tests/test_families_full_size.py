"""The Linear traffic family with the Lidar observation, and direct ego control with the Kinematics observation, at the headline
shape on the MI355X -- 4096 environments x 51 vehicles (highway-fast-v0, 50 vehicles, 4 lanes) -- with EVERY environment stepped
through the oracle (tests/golden_util.py: OraclePool) and compared like in tests/families_util.py: rollout() (compare_step)."""
import numpy as np
import pytest

from highwayenv_amd import _abi
from oracle import oracle
from tests.families_util import comparable, compare_step, engine_state, make_engine
from tests.golden_util import OraclePool

STEPS = 5
CASES = {
    "linear-lidar": {"other_vehicles_type": "highway_env.vehicle.behavior.LinearVehicle",
                     "observation": {"type": "LidarObservation", "cells": 16}},
    "direct-kinematics": {"action": {"type": "DiscreteAction", "steering_range": [-0.1, 0.1]}},
}


def run_case(case, backend, E):
    cfg_d = _abi.highway_fast_default_config()
    cfg_d.update({"vehicles_count": 50, "lanes_count": 4}, **CASES[case])
    cfg = _abi.make_config(cfg_d, E, fast=True)
    assert cfg.num_vehicles == 51
    pool = OraclePool(E, lambda n: _abi.make_config(cfg_d, n, fast=True), threads=16)
    eng = make_engine(backend, cfg)
    eng.reset(base_seed=7000, ego_spacing=cfg_d["ego_spacing"], vehicles_density=cfg_d["vehicles_density"])  # device spawn (Philox)
    st = engine_state(eng)
    refs = pool.split(st)
    rng = np.random.default_rng(11)
    live = np.ones(E, bool)
    full = live_steps = 0
    for t in range(STEPS):
        acts = rng.integers(0, _abi.num_actions(cfg), size=(E, cfg.num_agents)).astype(np.int32)
        obs, reward, term, trunc, info = eng.step(acts)
        outs = pool.run(lambda c, mg, ref, a: oracle.step(c, ref, a), refs, pool.rows(acts))
        o2, r2, te2, tr2 = (np.concatenate([o[0][j] for o in outs]) for j in range(4))
        margin = np.concatenate([o[1] for o in outs])
        ref = {k: np.concatenate([r[k] for r in refs]) for k in refs[0]}
        wreck, ok = comparable(ref, margin, live)
        compare_step(cfg, eng, (obs, reward, term, trunc), ref, (o2, r2, te2, tr2), wreck, ok, live, f"{case} step {t}")
        full += int(ok.sum())
        live_steps += int(live.sum())
        live &= ~wreck
    eng.close()
    pool.close()
    print(f"\n{case}: {live_steps} live env-steps of {E * STEPS}, {full} compared in full, {live_steps - full} under the push-direction "
          f"exclusion; {int(live.sum())} environments wreck-free to the end")
    assert full >= 0.9 * live_steps and live_steps >= 0.5 * E * STEPS


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_headline_shape_every_environment_vs_oracle(case):
    run_case(case, "hip", 4096)
