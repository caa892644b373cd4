"""TEST INFRASTRUCTURE ONLY: the continuous entry points on the CPU emulation (tests/emu/emu_continuous.cpp).

``ContinuousEmuEngine`` is ``emu.EmuEngine`` (with ``SameStepEmuEngine``'s ``step_same_step``) plus the emulation's forms of
``Engine.act_continuous`` / ``step_continuous`` / ``rollout_continuous`` / ``step_same_step_continuous_device``: the product's
validation and launch rule (csrc/hwy_act.h, csrc/hwy_launch_units.h: select_act_continuous) and its act kernel run from one library
of their own (the unit ``continuous`` registered with ``emu.UNITS`` below, so that ``emu.build`` / ``emu.load`` and the mutation
builds treat it like the other units); the step behind the act launch is the direct family's own driver's with NO action ids.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from highwayenv_amd import _abi
from tests.emu import emu
from tests.emu.emu_same_step import SameStepEmuEngine

emu.UNITS["continuous"] = (["emu_continuous.cpp"], ["hwy_act.h", "hwy_launch_units.h"], "HWY_EMU_CONTINUOUS_LIB",
                           [("emu_continuous_config_size", _abi.HwyConfig), ("emu_continuous_params_size", _abi.HwyContinuousParams)],
                           "emu_continuous")


def _check(rc: int, L):
    """Raise what the product's Engine raises for a status (engine.py: _check_continuous)."""
    if rc == _abi.HWY_ERR_ACTION:
        raise ValueError(emu.last_error("continuous", L))
    emu._check("continuous", rc, L)


class ContinuousEmuEngine(SameStepEmuEngine):
    #: another (mutated) library of the unit for this engine's calls
    continuous_lib = None
    _no_ids = False

    def _actions(self, params, actions, lead=()):
        return np.ascontiguousarray(np.asarray(actions, np.float32).reshape(*lead, self.E, self.A, params.size))

    def _act(self, params, a, validate_values: bool):
        """One act launch on float32 [E, A, size]; `validate_values`: the host-pointer door's check of the values."""
        L = self.continuous_lib or emu.lib("continuous")
        _check(L.emu_continuous_validate(C.byref(self.cfg), C.byref(params)), L)
        if validate_values:
            _check(L.emu_continuous_check_finite(emu._p(a, C.c_float), C.c_longlong(a.size)), L)
        _check(self._scheduled(L, lambda: L.emu_continuous_act(C.byref(self.cfg), C.byref(params), emu._p(a, C.c_float),
                                                              emu._p(self.extra, C.c_double))), L)

    def _run(self, mode, n_frames, actions, k_steps=0):
        # (the step launch behind an act launch: the family's driver with no ids, whatever the caller's sequence hands it)
        return super()._run(mode, n_frames, None if self._no_ids else actions, k_steps)

    def act_continuous(self, params, actions):
        self._act(params, self._actions(params, actions), True)

    def act_continuous_device(self, params, actions):
        """hwy_act_continuous_device: the values are not validated (a non-finite row keeps its stored pair)."""
        self._act(params, self._actions(params, actions), False)

    def step_continuous(self, params, actions, validate_values: bool = True):
        self._act(params, self._actions(params, actions), validate_values)
        obs, reward, term, trunc, info = self._run(1, self.cfg.frames_per_step, None)
        return (self.observe() if self.lidar else obs[0]), reward[0], term[0], trunc[0], {k: v[0] for k, v in info.items()}

    def rollout_continuous(self, params, actions):
        """hwy_rollout_continuous: K (act, step) pairs; the values of all K blocks are validated before anything runs."""
        a = self._actions(params, actions, lead=(-1,))
        L = self.continuous_lib or emu.lib("continuous")
        _check(L.emu_continuous_validate(C.byref(self.cfg), C.byref(params)), L)
        _check(L.emu_continuous_check_finite(emu._p(a, C.c_float), C.c_longlong(a.size)), L)
        outs = [self.step_continuous(params, a[k], validate_values=False) for k in range(a.shape[0])]
        info = {key: np.stack([o[4][key] for o in outs]) for key in outs[0][4]}
        return tuple(np.stack([o[j] for o in outs]) for j in range(4)) + (info,)

    def step_same_step_continuous(self, params, actions, without=()) -> dict:
        """hwy_step_same_step_continuous_device: the act launch, then hwy_step_same_step_device's sequence with no ids."""
        self._act(params, self._actions(params, actions), False)
        self._no_ids = True
        try:
            return self.step_same_step(np.zeros((self.E, self.A), np.int32), without=without)
        finally:
            self._no_ids = False
