"""TEST INFRASTRUCTURE ONLY: the direct-ego-control kernels of the product source on the CPU (tests/emu/emu_control.cpp).

``EmuControlEngine`` has the Python surface of ``highwayenv_amd.engine.Engine`` that the control tests use (state, stored
controls, step, frames, K-step rollout, device reset, auto-reset), so that tests/test_control_parity.py runs the same checks
against this emulation and against the HIP engine on the MI355X.  ``HWY_EMU_CONTROL_LIB`` names a prebuilt (mutated)
emulator instead (tests/test_control_mutations.py).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from highwayenv_amd import _abi

from . import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_LIB = os.path.join(_HERE, "_build", "libhwy_emu_control.so")
_lib = None


def build(force: bool = False) -> str:
    if os.environ.get("HWY_EMU_CONTROL_LIB"):
        return os.environ["HWY_EMU_CONTROL_LIB"]
    srcs = [os.path.join(_HERE, "emu_control.cpp"), os.path.join(_HERE, "hip_emu.h"),
            os.path.join(_ROOT, "highwayenv_amd", "csrc", "hwy_device.h"),
            os.path.join(_ROOT, "highwayenv_amd", "csrc", "hwy_wave.h"),
            os.path.join(_ROOT, "highwayenv_amd", "csrc", "hwy_math.h"),
            os.path.join(_ROOT, "highwayenv_amd", "csrc", "hwy_params.h"),
            os.path.join(_ROOT, "include", "hwy_engine.h")]
    stale = not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(s) for s in srcs)
    if force or stale:
        os.makedirs(os.path.dirname(_LIB), exist_ok=True)
        emu.compile_emulator(srcs[0], _LIB)
    return _LIB


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_control_config_size.restype = C.c_size_t
        assert _lib.emu_control_config_size() == C.sizeof(_abi.HwyConfig)
    return _lib


def _p(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


class EmuControlEngine(emu.Scheduled):
    def __init__(self, cfg: _abi.HwyConfig):
        assert cfg.ego_control == _abi.EGO_DIRECT
        self.cfg = cfg
        self.E, self.N, self.A = cfg.num_envs, cfg.num_vehicles, cfg.num_agents
        self.st = _abi.alloc_state(self.E, self.N)
        self.controls = np.zeros((2, self.E, self.A))  # acceleration | steering, the device layout
        self.done = np.zeros(self.E, np.uint8)
        self.episode = np.zeros(self.E, np.uint32)
        self.autoreset = (0, 0, 2.0, 1.0, -1)

    def close(self):
        pass

    def set_state(self, st):
        self.st = {k: np.array(st[k], copy=True) for k in _abi.STATE_F64 + _abi.STATE_I32 + ["time"]}
        self.done[:] = 0

    def get_state(self):
        return _abi.copy_state(self.st)

    def set_controls(self, acceleration, steering):
        self.controls = np.ascontiguousarray(np.stack([np.asarray(acceleration, np.float64).reshape(self.E, self.A),
                                                       np.asarray(steering, np.float64).reshape(self.E, self.A)]))

    def get_controls(self):
        return self.controls[0].copy(), self.controls[1].copy()

    def set_autoreset(self, enabled, base_seed=0, ego_spacing=2.0, vehicles_density=1.0, initial_lane_id=-1):
        self.autoreset = (int(enabled), int(base_seed), float(ego_spacing), float(vehicles_density), int(initial_lane_id))

    def _run(self, mode, n_frames, actions, k_steps=0):
        E, A = self.E, self.A
        K = max(k_steps, 1)
        acts = None if actions is None else np.ascontiguousarray(np.asarray(actions, np.int32).reshape(K, E, A))
        obs = np.zeros((K, E, A, *_abi.obs_shape(self.cfg)), np.float32)
        reward = np.zeros((K, E, A))
        term, trunc = np.zeros((K, E), np.uint8), np.zeros((K, E), np.uint8)
        speed, crashed = np.zeros((K, E, A)), np.zeros((K, E, A), np.uint8)
        s = _abi.state_struct(self.st)
        ar = self.autoreset
        rc = self._scheduled(lib(), lambda: lib().emu_control_run(
            C.byref(self.cfg), C.byref(s), _p(self.controls, C.c_double), _p(self.done, C.c_uint8), _p(self.episode, C.c_uint32),
            C.c_int(mode), C.c_int(n_frames), C.c_int(k_steps), _p(acts, C.c_int32), _p(obs, C.c_float), _p(reward, C.c_double),
            _p(term, C.c_uint8), _p(trunc, C.c_uint8), _p(speed, C.c_double), _p(crashed, C.c_uint8), C.c_int(ar[0]),
            C.c_uint64(ar[1]), C.c_double(ar[2]), C.c_double(ar[3]), C.c_int(ar[4])))
        assert rc == 0
        info = {"speed": speed, "crashed": (crashed & 1).astype(bool)}
        return obs, reward, term.astype(bool), trunc.astype(bool), info

    def step(self, actions):
        a = np.asarray(actions)
        if ((a < 0) | (a > _abi.num_actions(self.cfg) - 1)).any():
            raise IndexError("action id outside the throttle x steering table")
        obs, reward, term, trunc, info = self._run(1, self.cfg.frames_per_step, actions)
        return obs[0], reward[0], term[0], trunc[0], {k: v[0] for k, v in info.items()}

    def rollout(self, actions):
        """hwy_rollout_device: actions [K, E, A] -> outputs with a leading K axis, ONE multi-step launch."""
        K = np.asarray(actions).reshape(-1, self.E, self.A).shape[0]
        return self._run(1, self.cfg.frames_per_step, actions, k_steps=K)

    def step_frames(self, actions, n_frames):
        self._run(0, n_frames, actions)

    def observe(self):
        return self._run(2, 0, None)[0][0]

    def reset(self, seeds=None, mask=None, ego_spacing=2.0, vehicles_density=1.0, initial_lane_id=-1, base_seed=0):
        E, A = self.E, self.A
        obs = np.zeros((E, A, *_abi.obs_shape(self.cfg)), np.float32)
        sd = None if seeds is None else np.ascontiguousarray(seeds, np.uint64)
        mk = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        s = _abi.state_struct(self.st)
        rc = self._scheduled(lib(), lambda: lib().emu_control_reset(
            C.byref(self.cfg), C.byref(s), _p(self.controls, C.c_double), _p(self.done, C.c_uint8), _p(self.episode, C.c_uint32),
            _p(mk, C.c_uint8), _p(sd, C.c_uint64), C.c_uint64(base_seed), C.c_double(ego_spacing), C.c_double(vehicles_density),
            C.c_int(initial_lane_id), _p(obs, C.c_float)))
        assert rc == 0
        return obs
