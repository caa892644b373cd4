"""TEST INFRASTRUCTURE ONLY: the time-to-collision grid / finite-MDP planner kernel of the product source on the CPU
(tests/emu/emu_ttc.cpp).

``EmuTtcEngine`` has the Python surface of ``highwayenv_amd.engine.Engine`` that the planner tests use.  The simulation is the
family's own emulated engine (``EmuEngine`` for IDM traffic, ``EmuTrafficEngine`` for the Linear family, ``EmuLidarEngine`` under a
Lidar observation; ``EmuControlEngine`` for a direct-control ego, which the planner refuses), and ``ttc_grid`` / ``mdp_plan`` run
the kernel of ``hwy_ttc.h`` on the state the last call left behind, with the validation of ``ttc_validate`` in front of it like
``hwy_engine.hip``.  ``HWY_EMU_TTC_LIB`` names a prebuilt (mutated) library instead (tests/test_ttc_mutations.py).
``set_schedule`` puts the planner's launches (and the simulation's) under another fiber order of hip_emu.h
(tests/test_schedule_independence.py).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from highwayenv_amd import _abi

from . import emu
from .emu import _p

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_lib = None


def build(force: bool = False) -> str:
    if os.environ.get("HWY_EMU_TTC_LIB"):
        return os.environ["HWY_EMU_TTC_LIB"]
    out = emu.flagged(os.path.join(_HERE, "_build", "libhwy_emu_ttc.so"))
    csrc = os.path.join(_ROOT, "highwayenv_amd", "csrc")
    srcs = [os.path.join(_HERE, f) for f in ("emu_ttc.cpp", "hip_emu.h")] + [
        os.path.join(csrc, f) for f in ("hwy_ttc.h", "hwy_device.h", "hwy_math.h")] + [os.path.join(_ROOT, "include", "hwy_engine.h")]
    if force or not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        emu.compile_emulator(srcs[0], out, emu._EXTRA)
    return out


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_ttc_config_size.restype = C.c_size_t
        _lib.emu_ttc_params_size.restype = C.c_size_t
        _lib.emu_ttc_last_error.restype = C.c_char_p
        assert _lib.emu_ttc_config_size() == C.sizeof(_abi.HwyConfig)
        assert _lib.emu_ttc_params_size() == C.sizeof(_abi.HwyTtcParams)
    return _lib


def _check(rc: int):
    msg = lib().emu_ttc_last_error().decode()
    if rc == _abi.HWY_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    if rc != 0:
        from highwayenv_amd.engine import EngineError
        raise EngineError(f"status {rc}: {msg}")


def _host_state(st: dict) -> dict:
    return {k: np.ascontiguousarray(st[k]) for k in _abi.STATE_F64 + _abi.STATE_I32 + ["time"]}


def ttc_shape(cfg: _abi.HwyConfig, params: _abi.HwyTtcParams) -> tuple:
    return (cfg.num_target_speeds, cfg.lanes_count, params.time_steps)


def status(cfg: _abi.HwyConfig, params) -> int:
    """The status the entry points return for (config, params) before any launch (csrc/hwy_ttc.h: ttc_validate)."""
    return lib().emu_ttc_validate(C.byref(cfg), None if params is None else C.byref(params))


def _run(sched, call):
    return call() if sched is None else sched._scheduled(lib(), call)


def ttc_grid(cfg: _abi.HwyConfig, st: dict, params: _abi.HwyTtcParams, sched=None) -> np.ndarray:
    """The kernel on a host state: grid f32 [E, A, V, L, T].  `sched`: an emu.Scheduled whose schedule the launch runs under."""
    st = _host_state(st)
    s = _abi.state_struct(st)
    _check(status(cfg, params))  # (first: the shape of the outputs needs valid params)
    grid = np.full((cfg.num_envs, cfg.num_agents, *ttc_shape(cfg, params)), np.nan, np.float32)
    _check(_run(sched, lambda: lib().emu_ttc_grid(C.byref(cfg), C.byref(s), C.byref(params), _p(grid, C.c_float))))
    return grid


def mdp_plan(cfg: _abi.HwyConfig, st: dict, params: _abi.HwyTtcParams, return_q=False, return_grid=False, sched=None):
    st = _host_state(st)
    s = _abi.state_struct(st)
    _check(status(cfg, params))
    action = np.full((cfg.num_envs, cfg.num_agents), -1, np.int32)
    q = np.full((cfg.num_envs, cfg.num_agents, 5), np.nan, np.float64) if return_q else None
    grid = np.full((cfg.num_envs, cfg.num_agents, *ttc_shape(cfg, params)), np.nan, np.float32) if return_grid else None
    _check(_run(sched, lambda: lib().emu_mdp_plan(C.byref(cfg), C.byref(s), C.byref(params), _p(action, C.c_int32), _p(q, C.c_double),
                                                  _p(grid, C.c_float))))
    return action, q, grid


class EmuTtcEngine:
    def __init__(self, cfg: _abi.HwyConfig):
        assert cfg.scenario == _abi.SCENARIO_HIGHWAY
        self.cfg = cfg
        self.E, self.N, self.A = cfg.num_envs, cfg.num_vehicles, cfg.num_agents
        if cfg.obs_type == _abi.OBS_LIDAR:
            from .emu_lidar import EmuLidarEngine
            self.sim = EmuLidarEngine(cfg)
        elif cfg.traffic_model == _abi.TRAFFIC_LINEAR:
            from .emu_traffic import EmuTrafficEngine
            self.sim = EmuTrafficEngine(cfg)
        elif cfg.ego_control == _abi.EGO_DIRECT:
            from .emu_control import EmuControlEngine
            self.sim = EmuControlEngine(cfg)
        else:
            self.sim = emu.EmuEngine(cfg)
        self.sched = emu.Scheduled()   # of the planner's own launches

    def __getattr__(self, name):  # stepping, state, behaviour parameters, auto-reset: the simulation's own
        return getattr(self.sim, name)

    def ttc_shape(self, params):
        return ttc_shape(self.cfg, params)

    def set_schedule(self, **schedule):
        self.sim.set_schedule(**schedule)
        self.sched.set_schedule(**schedule)

    def schedule_errors(self) -> int:
        return self.sim.schedule_errors() + self.sched.schedule_errors()

    def schedule_error_text(self) -> str:
        return self.sim.schedule_error_text() or self.sched.schedule_error_text()

    def ttc_grid(self, params):
        return ttc_grid(self.cfg, self.sim.get_state(), params, self.sched)

    def mdp_plan(self, params, return_q=False, return_grid=False):
        return mdp_plan(self.cfg, self.sim.get_state(), params, return_q, return_grid, self.sched)
