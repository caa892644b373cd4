"""TEST INFRASTRUCTURE ONLY: the TimeToCollision observation's entry points on the CPU emulation (tests/emu/emu_ttc_obs.cpp).

``TtcObsEmuEngine`` is ``emu.EmuEngine`` (with ``SameStepEmuEngine``'s ``step_same_step``) plus the emulation's forms of
``Engine.ttc_observe`` / ``step_same_step_ttc_device`` / ``rollout_ttc_device``: the product's validation,
launch rule and sequences (csrc/hwy_collision_obs.h, csrc/hwy_launch_units.h: select_collision_obs) with the observation kernel and
the stash run from one library of their own (the unit ``ttc_obs`` registered with ``emu.UNITS`` below, so that ``emu.build`` /
``emu.load`` and the mutation builds treat it like the other units); the step launch, the mask kernel and the re-spawn are called
back from it, as the OPD unit calls back its step.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from highwayenv_amd import _abi
from tests.emu import emu
from tests.emu.emu_same_step import SENTINEL_F32, SENTINEL_F64, SENTINEL_U8, SameStepEmuEngine, new_planes

emu.UNITS["ttc_obs"] = (["emu_ttc_obs.cpp"],
                        ["hwy_collision_obs.h", "hwy_ttc.h", "hwy_same_step.h", "hwy_device.h", "hwy_math.h", "hwy_launch_units.h"],
                        "HWY_EMU_TTC_OBS_LIB", [("emu_ttc_obs_config_size", _abi.HwyConfig), ("emu_ttc_obs_params_size", _abi.HwyTtcParams)],
                        "emu_ttc_obs")


def ttc_obs_status(cfg: _abi.HwyConfig, params, L=None) -> int:
    """The status the entry points return for (config, params) before any launch (csrc/hwy_collision_obs.h: ttc_obs_validate);
    the reason: ``emu.last_error("ttc_obs")``."""
    return (L or emu.lib("ttc_obs")).emu_ttc_obs_validate(C.byref(cfg), None if params is None else C.byref(params))


def ttc_obs_rules(V, L, T, N=20, pitch=None, A=1, rows=4, with_arrays=True) -> tuple:
    """What select_collision_obs answers for a shape: (status, grid, block, dynamic LDS bytes)."""
    out = (C.c_int * 4)()
    emu.lib("ttc_obs").emu_ttc_obs_rules(*(C.c_int32(int(v)) for v in (V, L, T, N, N if pitch is None else pitch, A, rows)), int(with_arrays), out)
    return tuple(out)


def ttc_obs_sequence(final_action_mask: bool = False, action_mask: bool = False, k_steps: int = 0) -> list:
    """The operations of hwy_step_same_step_ttc_device (``k_steps`` 0) or hwy_rollout_ttc_device, in order, as words."""
    buf = C.create_string_buffer(1 << 14)
    assert emu.lib("ttc_obs").emu_ttc_obs_sequence(int(final_action_mask), int(action_mask), C.c_int32(k_steps), buf, C.c_int(len(buf))) == 0
    return buf.value.decode().split()


def ttc_observe(cfg: _abi.HwyConfig, st: dict, params: _abi.HwyTtcParams, L=None, sched=None) -> np.ndarray:
    """The observation kernel on a host state: f32 [E, A, 3, 3, T].  `L`: another (mutated) library."""
    L = L or emu.lib("ttc_obs")
    s = _abi.state_struct(emu._host_state(st))
    emu._check("ttc_obs", ttc_obs_status(cfg, params, L), L)
    obs = np.full((cfg.num_envs, cfg.num_agents, *_abi.ttc_obs_shape(params)), np.nan, np.float32)
    emu._check("ttc_obs", emu._run(sched, L, lambda: L.emu_ttc_obs_launch(C.byref(cfg), C.byref(s), C.byref(params), emu._p(obs, C.c_float))), L)
    assert not np.isnan(obs).any(), "the kernel left a cell unwritten"
    return obs


def _guard(fn, raised):
    def guarded(*args):
        try:
            fn(*args)
            return 0
        except BaseException as e:  # (an exception cannot cross the C frames)
            raised.append(e)
            return _abi.HWY_ERR_INVALID_ARG
    return guarded


class TtcObsEmuEngine(SameStepEmuEngine):
    #: another (mutated) library of the unit for this engine's calls (tests/test_ttc_obs_mutations.py)
    ttc_obs_lib = None

    def ttc_observe(self, params) -> np.ndarray:
        return ttc_observe(self.cfg, self.get_state(), params, self.ttc_obs_lib, self)

    ttc_observe_host = ttc_observe

    def step_ttc(self, params, actions):
        """hwy_rollout_ttc_device with K = 1: (obs [E, A, 3, 3, T], reward, terminated, truncated, info) of one step."""
        out = self.rollout_ttc(params, np.asarray(actions, np.int32).reshape(1, self.E, self.A))
        return tuple(o[0] for o in out[:4]) + ({k: v[0] for k, v in out[4].items()},)

    def rollout_ttc(self, params, actions):
        """hwy_rollout_ttc_device: actions [K, E, A] -> (obs [K, E, A, 3, 3, T], reward [K, E, A], terminated [K, E], truncated
        [K, E], info): K (step, observe) pairs in one call of the unit."""
        L = self.ttc_obs_lib or emu.lib("ttc_obs")
        emu._check("ttc_obs", ttc_obs_status(self.cfg, params, L), L)
        acts = np.ascontiguousarray(np.asarray(actions, np.int32).reshape(-1, self.E, self.A))
        K, E, A = acts.shape[0], self.E, self.A
        obs = np.full((K, E, A, *_abi.ttc_obs_shape(params)), SENTINEL_F32, np.float32)
        reward, term, trunc = np.full((K, E, A), SENTINEL_F64), np.zeros((K, E), bool), np.zeros((K, E), bool)
        info = {"speed": np.full((K, E, A), SENTINEL_F64), "crashed": np.zeros((K, E, A), bool), "arrived": np.zeros((K, E, A), bool)}
        raised = []

        def step(k):  # hwy_step_device on block k: no validation of the ids, the step's own observation is dropped
            _, r, te, tr, inf = self._run(1, self.cfg.frames_per_step, acts[k])
            reward[k], term[k], trunc[k] = r[0], te[0], tr[0]
            for key in info:
                info[key][k] = inf[key][0]

        s = _abi.state_struct(self.st)
        rc = self._scheduled(L, lambda: L.emu_ttc_obs_rollout(C.byref(self.cfg), C.byref(s), C.byref(params), C.c_int32(K),
                                                              emu._p(obs, C.c_float), C.CFUNCTYPE(C.c_int, C.c_int)(_guard(step, raised))))
        if raised:
            raise raised[0]
        emu._check("ttc_obs", rc, L)
        return obs, reward, term, trunc, info

    def step_same_step_ttc(self, params, actions, masks: bool = False, without=()) -> dict:
        """One call of hwy_step_same_step_ttc_device: the planes of ``emu_same_step.new_planes`` after it, ``obs`` and
        ``final_obs`` [E, A, 3, 3, T].  `without`: planes handed over as NULL."""
        L = self.ttc_obs_lib or emu.lib("ttc_obs")
        c, ar, p = self.cfg, self.autoreset, emu._p
        out = new_planes(c, masks)
        for k in ("obs", "final_obs"):
            out[k] = np.full((self.E, self.A, *_abi.ttc_obs_shape(params)) if ttc_obs_status(c, params, L) == 0 else (1,), SENTINEL_F32, np.float32)
        ptr = {k: None if k in without else v for k, v in out.items()}
        emu._check("ttc_obs", L.emu_ttc_obs_same_step_validate(C.byref(c), None if params is None else C.byref(params), int(ar[0]),
                                                               int(ptr["final_obs"] is not None), int(ptr["final_mask"] is not None)), L)
        if masks:
            emu._check("mask", emu.mask_status(c))
        acts = np.ascontiguousarray(np.asarray(actions, np.int32).reshape(self.E, self.A))
        raised = []
        s = _abi.state_struct(self.st)

        def step():  # hwy_step_device: the family's step launch with auto-reset on; its own observation is dropped
            _, reward, term, trunc, info = self._run(1, c.frames_per_step, acts)
            out["reward"][...], out["terminated"][...], out["truncated"][...] = reward[0], term[0], trunc[0]
            out["speed"][...], out["crashed"][...] = info["speed"][0], info["crashed"][0]

        def mask(final):
            out["final_action_mask" if final else "action_mask"][...] = self.action_mask()

        def respawn():
            # the family's re-spawn kernel as the same_step unit launches it: that unit's sequence with a step that does nothing and
            # planes of its own for the step's observation, whose stash and observation nobody reads
            L2, own = emu.lib("same_step"), new_planes(c, False)
            rc = self._scheduled(L2, lambda: L2.emu_same_step_run(
                C.byref(c), C.byref(s), p(self.extra, C.c_double), p(self.done, C.c_uint8), p(self.episode, C.c_uint32),
                p(own["obs"], C.c_float), p(out["reward"], C.c_double), p(out["terminated"], C.c_uint8), p(out["truncated"], C.c_uint8),
                p(out["speed"], C.c_double), p(out["crashed"], C.c_uint8), p(own["final_obs"], C.c_float), p(own["final_speed"], C.c_double),
                p(own["final_crashed"], C.c_uint8), p(own["final_mask"], C.c_uint8), None, None, C.c_uint64(ar[1]), C.c_double(ar[2]),
                C.c_double(ar[3]), C.c_int(ar[4]), C.CFUNCTYPE(C.c_int)(lambda: 0)))
            emu._check("same_step", rc, L2)

        cb0, cb1 = C.CFUNCTYPE(C.c_int), C.CFUNCTYPE(C.c_int, C.c_int)
        rc = self._scheduled(L, lambda: L.emu_ttc_obs_same_step(
            C.byref(c), C.byref(s), C.byref(params), p(self.done, C.c_uint8), p(ptr["obs"], C.c_float), p(ptr["final_obs"], C.c_float),
            p(ptr["speed"], C.c_double), p(ptr["final_speed"], C.c_double), p(ptr["crashed"], C.c_uint8), p(ptr["final_crashed"], C.c_uint8),
            p(ptr["final_mask"], C.c_uint8), int(masks), int(masks), cb0(_guard(step, raised)), cb1(_guard(mask, raised)),
            cb0(_guard(respawn, raised))))
        if raised:
            raise raised[0]
        emu._check("ttc_obs", rc, L)
        return out
