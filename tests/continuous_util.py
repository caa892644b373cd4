"""Shared helpers of the continuous-control tests: the NumPy restatement of the act kernel's mapping, the fixtures of
tests/golden/continuous and the backends (``emu`` = tests/emu/emu_continuous.py on the CPU, ``hip`` = the engine on the MI355X)."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

from highwayenv_amd import _abi
from tests.control_util import ControlGolden

CONTINUOUS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "continuous")
BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
FIXTURES = ["cont_fast", "cont_v0", "cont_asym", "cont_longi_only", "cont_lat_only", "cont_ma2", "cont_n100", "cont_throttle",
            "cont_dense"]

F32 = np.float32


def restate_axis(v, y0: float, y1: float) -> np.ndarray:
    """``utils.lmap(np.clip(v, -1, 1), [-1, 1], [y0, y1])`` of float32 values as NumPy 2 computes it, one operation at a time: the
    clip in float32, the difference of the range ends in double THEN rounded, three float32 operations each rounded on its own,
    the float32 add with the rounded lower end, the result widened to float64 (``Vehicle.clip_actions`` applies ``float()``)."""
    v = np.asarray(v, F32)
    x = np.minimum(np.maximum(v, F32(-1.0)), F32(1.0))
    r = F32(float(y1) - float(y0))
    s = (x + F32(1.0)).astype(F32)
    m = (s * r).astype(F32)
    t = (m / F32(2.0)).astype(F32)
    o = (F32(float(y0)) + t).astype(F32)
    return o.astype(np.float64)


def restate(params: _abi.HwyContinuousParams, actions, stored=None):
    """The (acceleration, steering) planes [..., ] the act kernel leaves for float32 ``actions`` [..., size]: an axis that is not
    controlled holds 0.0; a row with a non-finite component keeps ``stored`` = (acceleration, steering) (zeros when None)."""
    a = np.asarray(actions, F32)
    assert a.shape[-1] == params.size
    with np.errstate(invalid="ignore"):
        accel = restate_axis(a[..., 0], *params.acceleration_range) if params.longitudinal else np.zeros(a.shape[:-1])
        steer = restate_axis(a[..., -1], *params.steering_range) if params.lateral else np.zeros(a.shape[:-1])
    bad = ~np.isfinite(a).all(axis=-1)
    if bad.any():
        keep = (np.zeros_like(accel), np.zeros_like(steer)) if stored is None else stored
        accel, steer = np.where(bad, keep[0], accel), np.where(bad, keep[1], steer)
    return accel, steer


def params_of(action: dict) -> _abi.HwyContinuousParams:
    return _abi.continuous_params(action["action_config"] if action["type"] == "MultiAgentAction" else action)


def discrete_of(action: dict, actions_per_axis: int = 3) -> dict:
    """The ``DiscreteAction`` config with the ranges and axes of a ``ContinuousAction`` one (the engine's configuration)."""
    if action["type"] == "MultiAgentAction":
        return {"type": "MultiAgentAction", "action_config": discrete_of(action["action_config"], actions_per_axis)}
    assert action["type"] in ("ContinuousAction", "DiscreteAction")
    out = {k: v for k, v in action.items() if k != "type"}
    out.update(type="DiscreteAction", actions_per_axis=actions_per_axis)
    return out


def make_engine(backend: str, cfg):
    if backend == "emu":
        from tests.emu.emu_continuous import ContinuousEmuEngine
        return ContinuousEmuEngine(cfg)
    from highwayenv_amd.engine import Engine
    return Engine(cfg)


def emu_env_class(base):
    """`base` (a Batched*Env or a single-environment drop-in) on the CPU emulation, continuous entry points included."""
    from tests.emu.emu_continuous import ContinuousEmuEngine
    return type("Emu" + base.__name__, (base,), {"_engine_factory": staticmethod(lambda cfg, device, stream: ContinuousEmuEngine(cfg))})


def env_class(backend: str, base):
    return emu_env_class(base) if backend == "emu" else base


class ContinuousGolden(ControlGolden):
    """A fixture of tests/golden/continuous: make_golden_continuous.py's record of a ``ContinuousAction`` run of the reference.
    ``config["action"]`` is the matching ``DiscreteAction`` dict (what the engine is configured with), ``ref_action`` the
    reference's own; ``actions`` are float32 [steps, E, A, size]."""

    def __init__(self, name: str, data: dict | None = None):
        if data is None:
            with np.load(os.path.join(CONTINUOUS_DIR, name + ".npz")) as z:
                data = {k: z[k] for k in z.files}
        super().__init__(name, data)
        self.ref_action = json.loads(str(data["cfg_action_json"]))
        self.config["action"] = discrete_of(self.ref_action)
        self.params = params_of(self.ref_action)

    def actions_at(self, t: int) -> np.ndarray:
        return np.asarray(self.z["actions"][t], np.float32).reshape(self.E, self.A, self.params.size)


def assert_states_equal(sa: dict, sb: dict, what=""):
    for key in _abi.STATE_F64 + _abi.STATE_I32:
        np.testing.assert_array_equal(sa[key], sb[key], err_msg=f"{what}{key}")
