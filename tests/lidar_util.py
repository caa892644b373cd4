"""Shared helpers of the LidarObservation tests: the fixtures of tests/golden/lidar and the backends (``emu`` =
tests/emu/emu.py on the CPU, ``hip`` = the engine on the MI355X)."""
from __future__ import annotations

import json
import os

import numpy as np

from highwayenv_amd import _abi
from tests.backends import BACKENDS, make_engine  # noqa: F401  (re-exported)
from tests.golden_util import Golden

LIDAR_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lidar")
RUNS = ["lidar_fast", "lidar_v0", "lidar_cells64_raw", "lidar_ma2", "lidar_n100", "lidar_linear", "lidar_direct", "lidar_crash"]
FIXTURES = RUNS + ["lidar_crafted"]
OBS_ATOL = 1e-6  # the project's observation tolerance (an f32 ulp at 1 is 6e-8)


class LidarGolden(Golden):
    """A fixture of tests/golden/lidar: make_golden_lidar.py's record."""

    def __init__(self, name: str, data: dict | None = None):
        """`data`: the generator's arrays of a run (tests/test_lidar_live_reference.py) instead of the committed fixture."""
        if data is None:
            with np.load(os.path.join(LIDAR_DIR, name + ".npz")) as z:
                data = {k: z[k] for k in z.files}
        super().__init__(name, dict(data))
        self.A = int(data["cfg_controlled_vehicles"])
        self.config["controlled_vehicles"] = self.A
        self.config["other_vehicles_type"] = str(data["cfg_other_vehicles_type"])
        self.config["observation"] = json.loads(str(data["cfg_observation_json"]))
        self.config["action"] = json.loads(str(data["cfg_action_json"]))

    def hwy_config(self, num_envs=None, tuning=None) -> _abi.HwyConfig:
        return _abi.make_config(self.config, self.E if num_envs is None else num_envs, fast=self.fast, tuning=tuning)

    def actions_at(self, t: int) -> np.ndarray:
        return np.asarray(self.actions[t], np.int32).reshape(self.E, self.A)

    def load(self, eng, prefix: str = "init", index=None):
        """Put a recorded state on an engine: the planes, and what the family keeps beside them (the Linear family's drawn
        parameters, the stored controls of a direct-control ego)."""
        cfg = eng.cfg
        eng.set_state(self.state(prefix, index))
        if cfg.traffic_model == _abi.TRAFFIC_LINEAR:
            eng.set_behavior(self.z["init_behavior"])
        if cfg.ego_control == _abi.EGO_DIRECT:
            agents = list(cfg.agent_index[:self.A])
            a, s = (self.z[f"{prefix}_{k}"] if index is None else self.z[f"{prefix}_{k}"][index] for k in ("act_accel", "act_steering"))
            eng.set_controls(np.ascontiguousarray(a[:, agents]), np.ascontiguousarray(s[:, agents]))

    def reference_obs(self, index=None) -> np.ndarray:
        """[E, A, cells, 2]: the reference's observation at reset (None) or after step `index`."""
        return self.z["obs0"] if index is None else self.z["obs"][index]


def cells_off(got: np.ndarray, want: np.ndarray, atol: float = OBS_ATOL) -> int:
    """Number of (distance, velocity) cells that differ beyond `atol` in either component (a non-finite value differs)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(got - want) <= atol)
    return int(bad.any(axis=-1).sum())
