"""TEST INFRASTRUCTURE ONLY: the environment fork and the rollout scoring kernel of the product source on the CPU
(tests/emu/emu_lookahead.cpp).

``EmuLookaheadEngine`` has the Python surface of ``highwayenv_amd.engine.Engine`` that the lookahead tests and
``BatchedHighwayEnv.fork`` / ``score_sequences`` / ``plan_lookahead`` use.  The simulation is the family's own emulated engine (as in
``EmuTtcEngine``); ``fork_from`` (alias ``fork``) runs ``hwy_fork_kernel`` between the host arrays of two such engines,
``score`` runs ``hwy_score_kernel`` on the outputs of a rollout, and ``score_rollout`` is the two behind each other like
``hwy_score_rollout`` -- each with the validation of ``fork_validate`` / ``score_validate`` in front of it like ``hwy_engine.hip``.
``HWY_EMU_LOOKAHEAD_LIB`` names a prebuilt (mutated) library instead (tests/test_lookahead_mutations.py).  ``set_schedule`` puts
the two kernels' launches (and the simulation's) under another fiber order of hip_emu.h.
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
    if os.environ.get("HWY_EMU_LOOKAHEAD_LIB"):
        return os.environ["HWY_EMU_LOOKAHEAD_LIB"]
    out = emu.flagged(os.path.join(_HERE, "_build", "libhwy_emu_lookahead.so"))
    srcs = [os.path.join(_HERE, f) for f in ("emu_lookahead.cpp", "hip_emu.h")] + [
        os.path.join(_ROOT, "highwayenv_amd", "csrc", "hwy_lookahead.h"), os.path.join(_ROOT, "include", "hwy_engine.h")]
    if force or not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        emu.compile_emulator(srcs[0], out, emu._EXTRA)
    return out


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_lookahead_config_size.restype = C.c_size_t
        _lib.emu_lookahead_last_error.restype = C.c_char_p
        assert _lib.emu_lookahead_config_size() == C.sizeof(_abi.HwyConfig)
    return _lib


def _check(rc: int):
    msg = lib().emu_lookahead_last_error().decode()
    if rc == _abi.HWY_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    if rc != 0:
        from highwayenv_amd.engine import EngineError
        raise EngineError(f"status {rc}: {msg}")


def fork_status(dst_cfg, src_cfg, same_engine=False, branches=1, has_source=False) -> int:
    """The status hwy_fork_device returns for two configs before any launch (csrc/hwy_lookahead.h: fork_validate)."""
    return lib().emu_lookahead_fork_status(C.byref(dst_cfg), C.byref(src_cfg), int(same_engine), int(branches), int(has_source))


def _run(sched, call):
    return call() if sched is None else sched._scheduled(lib(), call)


def score(cfg, k_steps, branches, gamma, first_action, reward, terminated, truncated, want=("returns", "q", "best_action", "best_branch"),
          sched=None) -> dict:
    """hwy_score_device on host arrays (reward [K, E*B, A], flags [K, E*B], first_action [E*B, A] or None)."""
    K, B, A = int(k_steps), int(branches), cfg.num_agents
    E, ids = cfg.num_envs // max(B, 1), _abi.num_actions(cfg)
    rew = None if reward is None else np.ascontiguousarray(reward, np.float64)
    term = None if terminated is None else np.ascontiguousarray(terminated, np.uint8)
    trunc = None if truncated is None else np.ascontiguousarray(truncated, np.uint8)
    first = None if first_action is None else np.ascontiguousarray(first_action, np.int32)
    out = {"returns": np.full((E, max(B, 1), A), np.nan) if "returns" in want else None,
           "q": np.full((E, ids), np.nan) if "q" in want else None,
           "best_action": np.full(E, -1, np.int32) if "best_action" in want else None,
           "best_branch": np.full((E, A), -1, np.int32) if "best_branch" in want else None}
    _check(_run(sched, lambda: lib().emu_lookahead_score(
        C.byref(cfg), C.c_int32(K), C.c_int32(B), C.c_double(gamma), _p(first, C.c_int32), _p(rew, C.c_double), _p(term, C.c_uint8),
        _p(trunc, C.c_uint8), _p(out["returns"], C.c_double), _p(out["q"], C.c_double), _p(out["best_action"], C.c_int32),
        _p(out["best_branch"], C.c_int32))))
    return out


class EmuLookaheadEngine:
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
        self.sched = emu.Scheduled()   # of the two kernels' own launches

    def __getattr__(self, name):  # stepping, state, behaviour parameters, stored controls, auto-reset: the simulation's own
        return getattr(self.sim, name)

    def sync(self):
        pass

    def _core(self):
        """The engine that holds the arrays (a Lidar engine wraps its family's)."""
        return getattr(self.sim, "sim", self.sim)

    def set_schedule(self, **schedule):
        self._core().set_schedule(**schedule)
        self.sched.set_schedule(**schedule)

    def schedule_errors(self) -> int:
        return self._core().schedule_errors() + self.sched.schedule_errors()

    def schedule_error_text(self) -> str:
        return self._core().schedule_error_text() or self.sched.schedule_error_text()

    def _extra(self):
        core = self._core()
        return getattr(core, core.EXTRA) if getattr(core, "EXTRA", None) else None

    def fork_from(self, src: "EmuLookaheadEngine", branches: int = 1, source=None):
        idx = None
        if source is not None:
            idx = np.ascontiguousarray(source, dtype=np.int32)
            if idx.shape != (self.E,):
                raise ValueError(f"fork: source has shape {idx.shape}, this engine needs ({self.E},)")
        d, s = self._core(), src._core()
        sd, ss = _abi.state_struct(d.st), _abi.state_struct(s.st)
        _check(_run(self.sched, lambda: lib().emu_lookahead_fork(
            C.byref(self.cfg), C.byref(src.cfg), C.byref(sd), C.byref(ss), _p(self._extra(), C.c_double), _p(src._extra(), C.c_double),
            _p(d.done, C.c_uint8), _p(d.episode, C.c_uint32), _p(s.episode, C.c_uint32), C.c_int32(int(branches)), _p(idx, C.c_int32))))

    fork = fork_from

    def score(self, k_steps, branches, gamma, first_action, reward, terminated, truncated, **kw):
        return score(self.cfg, k_steps, branches, gamma, first_action, reward, terminated, truncated, sched=self.sched, **kw)

    def score_rollout(self, actions, branches: int, gamma: float = 1.0) -> dict:
        acts = np.ascontiguousarray(np.asarray(actions, np.int32).reshape(-1, self.E, self.A))
        K, A, B = acts.shape[0], self.A, int(branches)
        if B < 1 or self.E % B:
            raise ValueError(f"score_rollout: branches={B} does not divide the engine's {self.E} environments")
        if ((acts < 0) | (acts >= _abi.num_actions(self.cfg))).any():  # hwy_score_rollout: HWY_ERR_ACTION
            raise (IndexError if self.cfg.ego_control == _abi.EGO_DIRECT else KeyError)("action id out of range")
        _, reward, term, trunc, _ = self.sim.rollout(acts)
        want = ("returns", "q", "best_action", "best_branch") if A == 1 else ("returns", "best_branch")
        out = self.score(K, B, gamma, acts[0] if A == 1 else None, reward, term, trunc, want=want)
        out.update(reward=reward, terminated=term, truncated=trunc)
        return out
