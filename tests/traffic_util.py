"""Shared helpers of the LinearVehicle-family tests: the fixtures of tests/golden/traffic and the backends
(``emu`` = tests/emu/emu.py on the CPU, ``hip`` = the engine on the MI355X)."""
from __future__ import annotations

import json
import os

import numpy as np

from highwayenv_amd import _abi
from tests.backends import BACKENDS, make_engine  # noqa: F401  (re-exported)
from tests.golden_util import Golden

TRAFFIC_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "traffic")
FIXTURES = ["linear_fast", "linear_v0", "aggressive_dense", "defensive_ma2", "linear_n100", "crash_many_linear"]


class TrafficGolden(Golden):
    """A fixture of tests/golden/traffic: make_golden.py's record plus the traffic class and the drawn parameters."""

    def __init__(self, name: str, data: dict | None = None):
        """`data`: the generator's arrays of a run (tests/test_traffic_live_reference.py) instead of the committed fixture."""
        if data is None:
            with np.load(os.path.join(TRAFFIC_DIR, name + ".npz")) as z:
                data = {k: z[k] for k in z.files}
        data = dict(data)
        A = int(data["cfg_controlled_vehicles"])
        for k in ("cfg_normalize_reward", "cfg_offroad_terminal", "cfg_collision_reward", "cfg_right_lane_reward",
                  "cfg_high_speed_reward", "cfg_reward_speed_range"):
            if k not in data:  # (the multi-agent record keeps the class defaults)
                d = _abi.highway_default_config()[k[4:]]
                data[k] = np.asarray(d)
        super().__init__(name, data)
        self.A = A
        self.config["other_vehicles_type"] = str(data["cfg_other_vehicles_type"])
        self.config["controlled_vehicles"] = A
        if A > 1:
            self.config["observation"] = json.loads(str(data["cfg_observation_json"]))
            self.config["action"] = json.loads(str(data["cfg_action_json"]))
        self.behavior = data["init_behavior"]

    def hwy_config(self, num_envs=None, tuning=None) -> _abi.HwyConfig:
        return _abi.make_config(self.config, self.E if num_envs is None else num_envs, fast=self.fast, tuning=tuning)

    def actions_at(self, t: int) -> np.ndarray:
        return np.asarray(self.actions[t], np.int32).reshape(self.E, self.A)
