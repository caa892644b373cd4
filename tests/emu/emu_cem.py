"""TEST INFRASTRUCTURE ONLY: the float door into fork / rollout / score and the CEM planner on the CPU emulation
(tests/emu/emu_cem.cpp).

``CemEmuEngine`` is ``ContinuousEmuEngine`` plus the emulation's forms of ``Engine.score_rollout_continuous`` and
``Engine.cem_plan``: the product's validation (csrc/hwy_cem.h: cem_validate), launch rules (csrc/hwy_launch_units.h) and sequence
(cem_iterate) with the two CEM kernels, the fork and the fold run from one library of their own (the unit ``cem`` registered with
``emu.UNITS`` below, so that ``emu.build`` / ``emu.load`` and the mutation builds treat it like the other units); the work engine's
K (act, step) pairs are called back from it, as the OPD unit calls back its step.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from highwayenv_amd import _abi
from tests.emu import emu
from tests.emu.emu_continuous import ContinuousEmuEngine, _check as _check_continuous


class _CemArrays(C.Structure):  # hwy_cem.h: CemArrays
    _fields_ = [(k, C.c_void_p) for k in ("actions", "init_mean", "mean", "std", "noise", "samples", "best_return", "best_sequence", "action", "elites")]


emu.UNITS["cem"] = (["emu_cem.cpp", "emu_fork.h"],
                    ["hwy_cem.h", "hwy_act.h", "hwy_lookahead.h", "hwy_device.h", "hwy_math.h", "hwy_launch_units.h"], "HWY_EMU_CEM_LIB",
                    [("emu_cem_config_size", _abi.HwyConfig), ("emu_cem_continuous_size", _abi.HwyContinuousParams),
                     ("emu_cem_params_size", _abi.HwyCemParams), ("emu_cem_arrays_size", _CemArrays)], "emu_cem")


def _check(rc: int, L):
    """Raise what the product's Engine raises for a status (engine.py: _check_continuous)."""
    if rc == _abi.HWY_ERR_ACTION:
        raise ValueError(emu.last_error("cem", L))
    emu._check("cem", rc, L)


def cem_validate(src_cfg, work_cfg, cp, params, has_action=True, L=None) -> int:
    """The status hwy_cem_plan_device returns before any launch (csrc/hwy_cem.h: cem_validate); the reason: ``last_error("cem")``."""
    L = L or emu.lib("cem")
    return L.emu_cem_validate(C.byref(src_cfg), C.byref(work_cfg), None if cp is None else C.byref(cp),
                              None if params is None else C.byref(params), int(has_action))


def cem_sequence(iterations: int, population: int, horizon: int) -> list:
    """The operations hwy_cem.h's cem_iterate -- the sequence of hwy_cem_plan_device -- runs, in order, as words."""
    buf = C.create_string_buffer(1 << 16)
    assert emu.lib("cem").emu_cem_sequence(C.c_int32(iterations), C.c_int32(population), C.c_int32(horizon), buf, C.c_int(len(buf))) == 0
    return buf.value.decode().split()


def cem_rules(E, B, K, size, M, I, it=0, with_arrays=True) -> dict:
    """What select_cem_sample / select_cem_refit answer for a shape: {"sample": (status, grid, block), "refit": (...)}."""
    s, r = (C.c_int * 3)(), (C.c_int * 3)()
    emu.lib("cem").emu_cem_rules(*(C.c_int32(int(v)) for v in (E, B, K, size, M, I, it)), int(with_arrays), s, r)
    return {"sample": tuple(s), "refit": tuple(r)}


def cem_uniform2(seed: int, env: int, branch: int, draw: int, L=None) -> tuple:
    """The two uniforms the sample kernel takes from its Philox block (csrc/hwy_cem.h: cem_uniform2)."""
    u0, u1 = C.c_double(), C.c_double()
    (L or emu.lib("cem")).emu_cem_uniform2(C.c_uint64(seed), C.c_uint32(env), C.c_uint32(branch), C.c_uint32(draw), C.byref(u0), C.byref(u1))
    return u0.value, u1.value


def cem_sample(cp, cem, num_envs: int, iteration: int = 0, mean=None, std=None, L=None, sched=None) -> dict:
    """One launch of the sample kernel alone: ``noise`` f64 / ``samples`` f32 [E, B, K, size] of iteration ``iteration`` around
    ``mean`` / ``std`` [E, K, size] (iteration 0: zeros / init_std)."""
    L = L or emu.lib("cem")
    E, B, K, size = int(num_envs), cem.population, cem.horizon, cp.size
    lead = iteration + 1  # (the debug planes are indexed by the iteration)
    noise, samples = np.full((lead, E, B, K, size), np.nan), np.full((lead, E, B, K, size), np.nan, np.float32)
    actions = np.full((K, E * B, size), np.nan, np.float32)
    mean = np.zeros((E, K, size)) if mean is None else np.ascontiguousarray(mean, np.float64)
    std = np.full((E, K, size), cem.init_std) if std is None else np.ascontiguousarray(std, np.float64)
    a = _CemArrays(actions.ctypes.data, None, mean.ctypes.data, std.ctypes.data, noise.ctypes.data, samples.ctypes.data, None, None, None, None)
    _check(emu._run(sched, L, lambda: L.emu_cem_sample(C.byref(cp), C.byref(cem), C.c_int32(E), C.c_int32(iteration), C.byref(a))), L)
    return {"noise": noise[iteration], "samples": samples[iteration], "actions": actions}


class CemEmuEngine(ContinuousEmuEngine):
    #: another (mutated) library of the unit for this engine's plans (tests/test_cem_mutations.py)
    cem_lib = None

    def score_rollout_continuous(self, params, actions, branches: int, gamma: float = 1.0) -> dict:
        """hwy_score_rollout_continuous: the validation, K (act, step) pairs, the fold with no first action."""
        a = self._actions(params, actions, lead=(-1,))
        K, B = a.shape[0], int(branches)
        if B < 1 or self.E % B:
            raise ValueError(f"score_rollout_continuous: branches={B} does not divide the engine's {self.E} environments")
        L = self.continuous_lib or emu.lib("continuous")
        _check_continuous(L.emu_continuous_validate(C.byref(self.cfg), C.byref(params)), L)
        emu._check("lookahead", emu.lib("lookahead").emu_lookahead_score_status(
            C.byref(self.cfg), C.c_int32(K), C.c_int32(B), C.c_double(gamma), 0, 1, 0, 0))
        _check_continuous(L.emu_continuous_check_finite(emu._p(a, C.c_float), C.c_longlong(a.size)), L)
        outs = [self.step_continuous(params, a[k], validate_values=False) for k in range(K)]
        reward, term, trunc = (np.stack([o[j] for o in outs]) for j in (1, 2, 3))
        scored = self.score(K, B, gamma, None, reward, term, trunc, want=("returns", "best_branch"))
        out = {k: scored[k] for k in ("returns", "best_branch")}  # (a float sequence has no first action id: no q, no best_action)
        out.update(reward=reward, terminated=term, truncated=trunc)
        return out

    def cem_plan(self, work: "CemEmuEngine", params, cem, init_mean=None, debug: bool = False) -> dict:
        """hwy_cem_plan: the validation, then ONE call of the CEM unit that runs the product's sequence (hwy_cem.h: cem_iterate)."""
        L = self.cem_lib or emu.lib("cem")
        _check(cem_validate(self.cfg, work.cfg, params, cem, True, L), L)
        if work is self:
            raise ValueError("src and work must be two engines")
        if work.autoreset[0]:
            from highwayenv_amd.engine import EngineError
            raise EngineError("status -1: hwy_cem_plan: work must run with auto-reset off")
        E, B, K, I, size = self.E, cem.population, cem.horizon, cem.iterations, params.size
        im = None
        if init_mean is not None:
            im = np.ascontiguousarray(init_mean, dtype=np.float64)
            if im.shape != (E, K, size):
                raise ValueError(f"cem_plan: init_mean has shape {im.shape}, this search needs {(E, K, size)}")
            _check(L.emu_cem_check_finite(emu._p(im, C.c_double), C.c_longlong(im.size)), L)
        return self._cem_launch(work, params, cem, im, debug)

    def _cem_launch(self, work, params, cem, im, debug, without=()):
        """The launches behind a passed validation; `without`: arrays handed over as NULL (what the launch rules refuse)."""
        L = self.cem_lib or emu.lib("cem")
        E, B, K, I, size = self.E, cem.population, cem.horizon, cem.iterations, params.size
        out = {"action": np.full((E, size), np.nan, np.float32), "best_return": np.full(E, np.nan), "mean": np.full((E, K, size), np.nan),
               "std": np.full((E, K, size), np.nan), "best_sequence": np.full((E, K, size), np.nan, np.float32),
               "noise": np.full((I, E, B, K, size), np.nan) if debug else None,
               "samples": np.full((I, E, B, K, size), np.nan, np.float32) if debug else None,
               "elites": np.full((I, E, cem.elites), -7, np.int32) if debug else None}
        actions = np.full((K, E * B, 1, size), np.nan, np.float32)
        ret = np.full(E * B, np.nan)
        reward, term, trunc = np.full((K, E * B), np.nan), np.zeros((K, E * B), np.uint8), np.zeros((K, E * B), np.uint8)
        raised = []

        def rollout():  # hwy_rollout_continuous_device: no validation of the values, no copy of the observation
            try:
                for k in range(K):
                    _, r, te, tr, _ = work.step_continuous(params, actions[k], validate_values=False)
                    reward[k], term[k], trunc[k] = r[:, 0], te, tr
                return 0
            except BaseException as e:  # (an exception cannot cross the C frames)
                raised.append(e)
                return _abi.HWY_ERR_INVALID_ARG

        arrays = {"actions": actions, "init_mean": im, "mean": out["mean"], "std": out["std"], "noise": out["noise"], "samples": out["samples"],
                  "best_return": out["best_return"], "best_sequence": out["best_sequence"], "action": out["action"], "elites": out["elites"]}
        a = _CemArrays(*(None if (k in without or arrays[k] is None) else arrays[k].ctypes.data for k, _ in _CemArrays._fields_))
        (sv, _s), (wv, _w) = self._view(), work._view()
        cb = C.CFUNCTYPE(C.c_int)(rollout)
        rc = self._scheduled(L, lambda: L.emu_cem_plan(C.byref(sv), C.byref(wv), C.byref(params), C.byref(cem), C.byref(a),
                                                       emu._p(ret, C.c_double), emu._p(reward, C.c_double), emu._p(term, C.c_uint8),
                                                       emu._p(trunc, C.c_uint8), cb))
        if raised:
            raise raised[0]
        _check(rc, L)
        self.last_cem_returns = ret.reshape(E, B).copy()  # (of the last iteration)
        return out
