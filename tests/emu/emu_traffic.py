"""TEST INFRASTRUCTURE ONLY: the Linear traffic family's kernels of the product source on the CPU (tests/emu/emu_traffic.cpp).

``EmuTrafficEngine`` has the Python surface of ``highwayenv_amd.engine.Engine`` that the traffic tests use (state, behaviour
parameters, step, frames, K-step rollout, device reset, auto-reset, math probes), so that tests/test_traffic_parity.py runs
the same checks against this emulation and against the HIP engine on the MI355X.  ``HWY_EMU_TRAFFIC_LIB`` names a prebuilt
(mutated) emulator instead (tests/test_families_mutations.py).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from highwayenv_amd import _abi

from . import emu
from .emu import _p


class EmuTrafficEngine(emu.StraightFamilyEngine):
    SOURCE, SYMBOL, ENV, EXTRA = "emu_traffic.cpp", "emu_traffic", "HWY_EMU_TRAFFIC_LIB", "planes"
    BAD_ACTION = (KeyError, "invalid meta-action")

    def __init__(self, cfg: _abi.HwyConfig):
        assert cfg.traffic_model == _abi.TRAFFIC_LINEAR
        super().__init__(cfg)
        self.planes = np.zeros((_abi.HWY_BEHAVIOR_PARAMS, self.E, self.N))  # the device layout [k][E][N]

    def set_behavior(self, params):
        a = np.asarray(params, np.float64)
        assert a.shape == (self.E, self.N, _abi.HWY_BEHAVIOR_PARAMS)
        self.planes = np.ascontiguousarray(a.transpose(2, 0, 1))

    def get_behavior(self):
        return np.ascontiguousarray(self.planes.transpose(1, 2, 0))

    def debug_math(self, op, x):
        xin = np.ascontiguousarray(x, np.float64).ravel()
        out = np.empty_like(xin)
        self.lib().emu_traffic_debug_math(C.c_int(op), _p(xin, C.c_double), _p(out, C.c_double), C.c_longlong(xin.size))
        return out.reshape(np.shape(x))


build, lib = EmuTrafficEngine.build, EmuTrafficEngine.lib


def behavior_draw(seed: int, vehicle: int, episode: int) -> np.ndarray:
    """The device's Philox draw of one vehicle's parameters (hwy_device.h: linear_behavior_draw)."""
    out = np.zeros(_abi.HWY_BEHAVIOR_PARAMS)
    lib().emu_traffic_behavior_draw(C.c_uint64(seed), C.c_int(vehicle), C.c_uint32(episode), _p(out, C.c_double))
    return out
