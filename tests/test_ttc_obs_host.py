"""Host side of the TimeToCollision observation (no GPU): what the entry points refuse (csrc/hwy_collision_obs.h: ttc_obs_validate,
through the emulation's build of it) with status and reason, NULL arguments, the ABI that stays as it was, the launch rule's grid /
block / LDS (csrc/hwy_launch_units.h: select_collision_obs) and the two sequences of launches as words."""
import ctypes as C
import os

import numpy as np
import pytest

from highwayenv_amd import _abi, _lib
from tests import ttc_util
from tests.emu import emu, emu_ttc_obs

NEW = ["hwy_ttc_observe_device", "hwy_ttc_observe", "hwy_step_same_step_ttc_device", "hwy_rollout_ttc_device"]
DIRECT = {"type": "DiscreteAction"}


def _cfg(**over):
    return _abi.make_config(ttc_util.highway_config(**over), 2, fast=True)


def _one_speed():
    """One target speed: the front end's make_config refuses the list, the C-ABI's hwy_config can say it."""
    c = _cfg()
    c.num_target_speeds = 1
    return c


def _params(built_for=10.0, **fields):
    """hwy_ttc_params of highway-fast-v0 for the horizon `built_for`, then `fields` overwritten as they are."""
    p = _abi.ttc_params(ttc_util.highway_config(), horizon=built_for)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _status(cfg, params):
    return emu_ttc_obs.ttc_obs_status(cfg, params), emu.last_error("ttc_obs")


def test_what_is_accepted():
    assert _status(_cfg(), _params()) == (0, "")
    for action in ({"type": "DiscreteMetaAction", "lateral": False}, {"type": "DiscreteMetaAction", "longitudinal": False}):
        assert _status(_cfg(action=action), _params())[0] == 0, "any action_set"      # (the planner refuses these)
    assert _status(_cfg(action={"type": "DiscreteMetaAction", "target_speeds": [20.0, 30.0]}), _params())[0] == 0
    assert _status(_cfg(other_vehicles_type="highway_env.vehicle.behavior.LinearVehicle"), _params())[0] == 0
    assert _status(_cfg(observation={"type": "LidarObservation", "cells": 16}), _params())[0] == 0
    # gamma and lane_change_reward are not read by this door
    assert _status(_cfg(), _params(gamma=float("nan"), lane_change_reward=float("inf")))[0] == 0
    assert emu.ttc_status(_cfg(), _params(gamma=float("nan"))) == _abi.HWY_ERR_INVALID_ARG  # (the planner's door reads them)
    assert _status(_cfg(), _params(built_for=1.0))[0] == 0 and _params(built_for=64.0).time_steps == _abi.HWY_MAX_TTC_STEPS


def test_every_refusal_with_its_status_and_reason():
    unsupported, invalid = _abi.HWY_ERR_UNSUPPORTED, _abi.HWY_ERR_INVALID_ARG
    from highwayenv_amd import intersection, merge
    rc, why = _status(_abi.make_config(merge.merge_default_config(), 2, scenario="merge"), _params())
    assert rc == unsupported and "highway scenario only" in why
    rc, why = _status(_abi.make_config(intersection.intersection_default_config(), 2, scenario="intersection"), _params())
    assert rc == unsupported and "highway scenario only" in why
    rc, why = _status(_cfg(action=DIRECT), _params())
    assert rc == unsupported and "DiscreteMetaAction" in why and "speed_index" in why
    rc, why = _status(_one_speed(), _params())
    assert rc == unsupported and "at least 2 target speeds" in why and "(2, 3, T)" in why
    rc, why = _status(_cfg(), None)
    assert rc == invalid and "NULL" in why
    for fields, reason in ((dict(time_steps=9), "int(horizon / time_quantization)"), (dict(time_steps=11), "int(horizon / time_quantization)"),
                           (dict(time_steps=0), "[1,64]"), (dict(time_steps=65, horizon=65.0), "[1,64]"),
                           (dict(time_quantization=0.0), "positive"), (dict(time_quantization=-1.0), "positive"),
                           (dict(time_quantization=float("nan")), "finite"), (dict(horizon=float("inf")), "finite"),
                           (dict(horizon=-1.0), "finite")):
        rc, why = _status(_cfg(), _params(**fields))
        assert rc == invalid and reason in why, (fields, rc, why)


def test_the_python_scope_check_states_the_same_rules():
    _abi.check_ttc_observation_scope(_cfg())
    from highwayenv_amd import merge
    for cfg in (_abi.make_config(merge.merge_default_config(), 2, scenario="merge"), _cfg(action=DIRECT),
                _one_speed()):
        assert emu_ttc_obs.ttc_obs_status(cfg, _params()) == _abi.HWY_ERR_UNSUPPORTED
        with pytest.raises(NotImplementedError):
            _abi.check_ttc_observation_scope(cfg)
    assert _abi.ttc_obs_shape(_params()) == (3, 3, 10)


def test_abi_stays_and_the_symbols_are_declared():
    lib = _lib.load()
    assert lib.hwy_abi_version() == _abi.HWY_ABI_VERSION == 8
    assert lib.hwy_config_size() == C.sizeof(_abi.HwyConfig) == emu.lib("ttc_obs").emu_ttc_obs_config_size()
    assert C.sizeof(_abi.HwyTtcParams) == 40 == emu.lib("ttc_obs").emu_ttc_obs_params_size() == emu.lib("ttc").emu_ttc_params_size()
    header = open(os.path.join(os.path.dirname(_abi.__file__), "..", "include", "hwy_engine.h")).read()
    assert "#define HWY_ABI_VERSION 8" in header
    for name in NEW:
        assert name in _lib.EXPORTS and f"int {name}(" in header and hasattr(lib, name)
    assert "IGNORED" in header[header.index("TimeToCollision observation"):header.index("hwy_ttc_observe_device(")]


def test_a_null_engine_is_refused_by_every_entry_point():
    lib = _lib.load()
    p, buf = _params(), np.zeros(4096, np.float32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    assert lib.hwy_ttc_observe_device(None, C.byref(p), ptr) == _abi.HWY_ERR_INVALID_ARG
    assert lib.hwy_ttc_observe(None, C.byref(p), ptr) == _abi.HWY_ERR_INVALID_ARG
    assert lib.hwy_step_same_step_ttc_device(None, C.byref(p), *([ptr] * 13)) == _abi.HWY_ERR_INVALID_ARG
    assert lib.hwy_rollout_ttc_device(None, C.byref(p), 2, *([ptr] * 7)) == _abi.HWY_ERR_INVALID_ARG


@pytest.mark.gpu
def test_null_params_and_outputs_on_an_engine():
    import torch

    from highwayenv_amd.engine import Engine, EngineError
    eng = Engine(_cfg())
    eng.reset(seeds=np.arange(2, dtype=np.uint64))
    p = _params()
    out = torch.zeros((2, 1, 3, 3, 10), dtype=torch.float32, device="cuda")
    lib = _lib.load()
    assert lib.hwy_ttc_observe_device(eng._h, None, C.c_void_p(out.data_ptr())) == _abi.HWY_ERR_INVALID_ARG
    assert b"NULL" in lib.hwy_last_error(eng._h)
    assert lib.hwy_ttc_observe(eng._h, C.byref(p), None) == _abi.HWY_ERR_INVALID_ARG
    with pytest.raises(EngineError, match="obs must be non-NULL"):
        eng.ttc_observe_device(p, 0)
    with pytest.raises(EngineError, match="non-NULL"):
        eng.rollout_ttc_device(p, 1, 0, out.data_ptr(), 0, 0, 0)
    with pytest.raises(EngineError, match="k_steps"):
        eng.rollout_ttc_device(p, 0, out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr())
    with pytest.raises(EngineError, match="auto-reset must be enabled"):
        eng.step_same_step_ttc_device(p, *([out.data_ptr()] * 6), d_final_obs=out.data_ptr(), d_final_mask=out.data_ptr())
    eng.set_autoreset(True, base_seed=1)
    with pytest.raises(EngineError, match="final_obs and final_mask"):
        eng.step_same_step_ttc_device(p, *([out.data_ptr()] * 6))
    with pytest.raises(EngineError, match="int\\(horizon / time_quantization\\)"):
        eng.ttc_observe(_params(time_steps=9))
    eng.close()


def test_the_launch_rule():
    lds = emu.lib("ttc_obs").emu_ttc_obs_lds_bytes()
    assert lds == 9 * _abi.HWY_MAX_TTC_STEPS * 4 == 2304
    # one 64-wide workgroup per (environment, agent) row, static LDS only, for every accepted shape
    for V, L, T, N, A, rows in ((3, 3, 10, 21, 1, 4096), (2, 1, 1, 1, 1, 1), (8, 16, 64, 256, 2, 8), (3, 4, 50, 65, 4, 12)):
        assert emu_ttc_obs.ttc_obs_rules(V, L, T, N=N, A=A, rows=rows) == (0, rows, 64, 0), (V, L, T, N, A, rows)
    # ... and nothing is launched for arguments the kernel is not built for
    for bad in (dict(V=1), dict(V=9), dict(L=0), dict(L=17), dict(T=0), dict(T=65), dict(N=0), dict(N=257), dict(N=21, pitch=20), dict(rows=0),
                dict(A=0), dict(A=3, rows=4), dict(with_arrays=False)):
        shape = dict(dict(V=3, L=3, T=10), **bad)
        assert emu_ttc_obs.ttc_obs_rules(**shape) == (-2, 0, 0, 0), bad


def test_the_sequences_as_words():
    seq = emu_ttc_obs.ttc_obs_sequence
    assert seq() == "step observe stash respawn observe".split()
    assert seq(final_action_mask=True, action_mask=True) == "step mask(final) observe stash respawn observe mask".split()
    assert seq(action_mask=True) == "step observe stash respawn observe mask".split()
    assert seq(k_steps=3) == "step(0) observe(0) step(1) observe(1) step(2) observe(2)".split()
