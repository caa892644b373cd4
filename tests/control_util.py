"""Shared helpers of the direct-ego-control (``DiscreteAction``) tests: the fixtures of tests/golden/control and the backends
(``emu`` = tests/emu/emu.py on the CPU, ``hip`` = the engine on the MI355X)."""
from __future__ import annotations

import json
import os

import numpy as np

from highwayenv_amd import _abi
from tests.backends import BACKENDS, make_engine  # noqa: F401  (re-exported)
from tests.golden_util import Golden

CONTROL_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "control")
FIXTURES = ["direct_fast", "direct_v0", "direct_k5", "direct_throttle", "direct_brake", "direct_offroad", "direct_offroad_terminal",
            "direct_longi_only", "direct_lat_only", "direct_ma2", "direct_n100", "direct_crash_many", "direct_rival"]
WITH_FRAMES = [n for n in FIXTURES if n not in ("direct_offroad_terminal", "direct_crash_many", "direct_rival")]


class ControlGolden(Golden):
    """A fixture of tests/golden/control: make_golden_control.py's record."""

    def __init__(self, name: str, data: dict | None = None):
        """`data`: the generator's arrays of a run (tests/test_control_live_reference.py) instead of the committed fixture."""
        if data is None:
            with np.load(os.path.join(CONTROL_DIR, name + ".npz")) as z:
                data = {k: z[k] for k in z.files}
        super().__init__(name, dict(data))
        self.A = int(data["cfg_controlled_vehicles"])
        self.config["controlled_vehicles"] = self.A
        self.config["observation"] = json.loads(str(data["cfg_observation_json"]))
        self.config["action"] = json.loads(str(data["cfg_action_json"]))

    def hwy_config(self, num_envs=None, tuning=None) -> _abi.HwyConfig:
        return _abi.make_config(self.config, self.E if num_envs is None else num_envs, fast=self.fast, tuning=tuning)

    def actions_at(self, t: int) -> np.ndarray:
        return np.asarray(self.actions[t], np.int32).reshape(self.E, self.A)

    def controls(self, prefix: str, index=None, envs=None):
        """The agents' stored (acceleration, steering), [E, A] each, as `init_*` / `step_*[index]` / `frame_*[index]` record them."""
        agents = list(self.hwy_config().agent_index[:self.A])
        out = []
        for k in ("act_accel", "act_steering"):
            a = self.z[f"{prefix}_{k}"]
            if index is not None:
                a = a[index]
            if envs is not None:
                a = a[envs]
            out.append(np.ascontiguousarray(a[:, agents]))
        return out[0], out[1]
