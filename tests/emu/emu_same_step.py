"""TEST INFRASTRUCTURE ONLY: ``hwy_step_same_step_device`` on the CPU emulation (tests/emu/emu_same_step.cpp).

``SameStepEmuEngine`` is ``emu.EmuEngine`` plus ``step_same_step``, the emulation's form of ``Engine.step_same_step_device``: the
product's validation and sequence (csrc/hwy_same_step.h), its stash kernel and the re-spawn kernels of every family run from one
library of their own (the unit ``same_step`` registered with ``emu.UNITS`` below, so that ``emu.build`` / ``emu.load`` and the
mutation builds treat it like the other units); the step launch is the family's own driver's, handed in as a callback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from highwayenv_amd import _abi
from tests.emu import emu

emu.UNITS["same_step"] = (
    ["emu_same_step.cpp", "emu_straight.h"],
    ["hwy_same_step.h", "hwy_device.h", "hwy_wave.h", "hwy_wave2.h", "hwy_net.h", "hwy_ix.h", "hwy_math.h", "hwy_params.h", "hwy_lidar.h",
     "hwy_mask.h", "hwy_launch_family.h", "hwy_launch_rules.h", "hwy_launch_units.h"],
    "HWY_EMU_SAME_STEP_LIB", [("emu_same_step_config_size", _abi.HwyConfig)], "emu_same_step")

#: what the final planes hold before a call: rows of environments that did not end must still hold it afterwards, bit for bit
SENTINEL_F32 = np.float32(np.nan)
SENTINEL_F64 = np.float64(np.nan)
SENTINEL_U8 = 0xFF


def new_planes(cfg: _abi.HwyConfig, masks: bool) -> dict:
    """The output planes of one call as host arrays, every one pre-filled with a sentinel."""
    E, A, ids = cfg.num_envs, cfg.num_agents, _abi.num_actions(cfg)
    shape = (E, A, *_abi.obs_shape(cfg))
    out = {"obs": np.full(shape, SENTINEL_F32, np.float32), "reward": np.full((E, A), SENTINEL_F64), "terminated": np.full(E, SENTINEL_U8, np.uint8),
           "truncated": np.full(E, SENTINEL_U8, np.uint8), "speed": np.full((E, A), SENTINEL_F64), "crashed": np.full((E, A), SENTINEL_U8, np.uint8),
           "final_obs": np.full(shape, SENTINEL_F32, np.float32), "final_speed": np.full((E, A), SENTINEL_F64),
           "final_crashed": np.full((E, A), SENTINEL_U8, np.uint8), "final_mask": np.full(E, SENTINEL_U8, np.uint8)}
    if masks:
        out["action_mask"] = np.full((E, A, ids), SENTINEL_U8, np.uint8)
        out["final_action_mask"] = np.full((E, A, ids), SENTINEL_U8, np.uint8)
    return out


class SameStepEmuEngine(emu.EmuEngine):
    #: another (mutated) library of the unit for this engine's calls (tests/test_same_step_mutations.py)
    same_step_lib = None

    def step_same_step(self, actions, masks: bool = False, without=()) -> dict:
        """One call of hwy_step_same_step_device: the planes of ``new_planes`` after it.  `without`: planes handed over as NULL."""
        L = self.same_step_lib or emu.lib("same_step")
        c, ar = self.cfg, self.autoreset
        out = new_planes(c, masks)
        ptr = {k: None if k in without else v for k, v in out.items()}
        emu._check("same_step", L.emu_same_step_validate(C.byref(c), int(ar[0]), int(ptr["final_obs"] is not None),
                                                         int(ptr["final_mask"] is not None), int(masks)), L)
        acts = np.ascontiguousarray(np.asarray(actions, np.int32).reshape(self.E, self.A))
        raised = []

        def step():  # hwy_step_device: the family's step launch with auto-reset on, a Lidar engine's trace behind it
            try:
                obs, reward, term, trunc, info = self._run(1, c.frames_per_step, acts)
                out["obs"][...] = self.observe() if self.lidar else obs[0]
                out["reward"][...], out["terminated"][...], out["truncated"][...] = reward[0], term[0], trunc[0]
                out["speed"][...], out["crashed"][...] = info["speed"][0], info["crashed"][0]
                return 0
            except BaseException as e:  # (an exception cannot cross the C frames)
                raised.append(e)
                return _abi.HWY_ERR_INVALID_ARG

        s = _abi.state_struct(self.st)
        p = emu._p
        rc = self._scheduled(L, lambda: L.emu_same_step_run(
            C.byref(c), C.byref(s), p(self.extra, C.c_double), p(self.done, C.c_uint8), p(self.episode, C.c_uint32),
            p(ptr["obs"], C.c_float), p(ptr["reward"], C.c_double), p(ptr["terminated"], C.c_uint8), p(ptr["truncated"], C.c_uint8),
            p(ptr["speed"], C.c_double), p(ptr["crashed"], C.c_uint8), p(ptr["final_obs"], C.c_float), p(ptr["final_speed"], C.c_double),
            p(ptr["final_crashed"], C.c_uint8), p(ptr["final_mask"], C.c_uint8), p(ptr.get("action_mask"), C.c_uint8),
            p(ptr.get("final_action_mask"), C.c_uint8), C.c_uint64(ar[1]), C.c_double(ar[2]), C.c_double(ar[3]), C.c_int(ar[4]),
            C.CFUNCTYPE(C.c_int)(step)))
        if raised:
            raise raised[0]
        emu._check("same_step", rc, L)
        return out
