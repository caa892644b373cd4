"""TEST INFRASTRUCTURE ONLY: the optimistic planner's tree kernel of the product source on the CPU (tests/emu/emu_opd.cpp).

``EmuOpdEngine`` is ``EmuLookaheadEngine`` plus ``opd_plan`` with the signature of ``highwayenv_amd.engine.Engine.opd_plan``: the
validation of ``opd_validate`` and then, per expansion, what ``hwy_opd_plan_device`` enqueues on the device -- ``hwy_opd_kernel``,
the gather tree -> work, one step of the work engine (the family's own emulated engine) with the action plane the kernel wrote,
the scatter work -> tree -- and one more kernel launch for the plan.  The two forks are ``hwy_fork_kernel`` in its device form
(source indices not validated: -1 copies nothing).  ``HWY_EMU_OPD_LIB`` names a prebuilt (mutated) library instead
(tests/test_opd_mutations.py).  ``set_schedule`` puts the kernel's launches under another fiber order of hip_emu.h.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from highwayenv_amd import _abi

from . import emu
from .emu import _p
from .emu_lookahead import EmuLookaheadEngine

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_lib = None


def build(force: bool = False) -> str:
    if os.environ.get("HWY_EMU_OPD_LIB"):
        return os.environ["HWY_EMU_OPD_LIB"]
    out = emu.flagged(os.path.join(_HERE, "_build", "libhwy_emu_opd.so"))
    srcs = [os.path.join(_HERE, f) for f in ("emu_opd.cpp", "hip_emu.h")] + [
        os.path.join(_ROOT, "highwayenv_amd", "csrc", f) for f in ("hwy_opd.h", "hwy_lookahead.h")] + [
        os.path.join(_ROOT, "include", "hwy_engine.h")]
    if force or not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        emu.compile_emulator(srcs[0], out, emu._EXTRA)
    return out


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_opd_config_size.restype = C.c_size_t
        _lib.emu_opd_params_size.restype = C.c_size_t
        _lib.emu_opd_last_error.restype = C.c_char_p
        assert _lib.emu_opd_config_size() == C.sizeof(_abi.HwyConfig)
        assert _lib.emu_opd_params_size() == C.sizeof(_abi.HwyOpdParams)
        assert _lib.emu_opd_max_nodes() == _abi.HWY_OPD_MAX_NODES
    return _lib


def _check(rc: int):
    msg = lib().emu_opd_last_error().decode()
    if rc == _abi.HWY_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    if rc != 0:
        from highwayenv_amd.engine import EngineError
        raise EngineError(f"status {rc}: {msg}")


def validate(src_cfg, tree_cfg, work_cfg, params, has_action=True) -> int:
    """The status hwy_opd_plan_device returns before any launch (csrc/hwy_opd.h: opd_validate); the reason: ``last_error()``."""
    return lib().emu_opd_validate(C.byref(src_cfg), C.byref(tree_cfg), C.byref(work_cfg), None if params is None else C.byref(params),
                                  int(has_action))


def last_error() -> str:
    return lib().emu_opd_last_error().decode()


class EmuOpdEngine(EmuLookaheadEngine):
    def fork_device(self, src: "EmuOpdEngine", branches: int = 1, source=None):
        """hwy_fork_device: ``source`` int32 [E] stands for the device array of indices (not validated), None for j // branches."""
        idx = None if source is None else np.ascontiguousarray(source, dtype=np.int32)
        assert idx is None or idx.shape == (self.E,)
        d, s = self._core(), src._core()
        sd, ss = _abi.state_struct(d.st), _abi.state_struct(s.st)
        call = lambda: lib().emu_opd_fork_device(  # noqa: E731
            C.byref(self.cfg), C.byref(src.cfg), C.byref(sd), C.byref(ss), _p(self._extra(), C.c_double), _p(src._extra(), C.c_double),
            _p(d.done, C.c_uint8), _p(d.episode, C.c_uint32), _p(s.episode, C.c_uint32), C.c_int32(int(branches)), _p(idx, C.c_int32))
        _check(self.sched._scheduled(lib(), call))

    def opd_plan(self, tree: "EmuOpdEngine", work: "EmuOpdEngine", params: _abi.HwyOpdParams) -> dict:
        _check(validate(self.cfg, tree.cfg, work.cfg, params))
        if tree is self or work is self or tree is work:
            raise ValueError("src, tree and work must be three engines")
        if tree._core().autoreset[0] or work._core().autoreset[0]:
            raise ValueError("tree and work must run with auto-reset off")
        E, n, M = self.E, params.n_ids, params.nodes
        X = params.budget // n
        t = {"ret": np.full((E, M), np.nan), "disc": np.full((E, M), np.nan), "upper0": np.full((E, M), np.nan),
             "done": np.full((E, M), 0xff, np.uint8), "node": np.full((E, X), -7, np.int32), "gather": np.full(E * n, -7, np.int32),
             "scatter": np.full(E * M, -7, np.int32), "root": np.full(E * M, -7, np.int32), "actions": np.full(E * n, -7, np.int32)}
        reward, term, trunc = np.full(E * n, np.nan), np.zeros(E * n, np.uint8), np.zeros(E * n, np.uint8)
        out = {"action": np.full(E, -7, np.int32), "value": np.full(E, np.nan), "upper": np.full(E, np.nan),
               "sequence": np.full((E, X), -7, np.int32), "expanded": np.full(E, -7, np.int32)}

        def kernel(x):
            _check(self.sched._scheduled(lib(), lambda: lib().emu_opd_kernel(
                C.c_int32(E), C.c_int32(n), C.c_int32(X), C.c_int32(x), C.c_double(params.gamma), C.c_double(params.bound),
                _p(t["ret"], C.c_double), _p(t["disc"], C.c_double), _p(t["upper0"], C.c_double), _p(t["done"], C.c_uint8),
                _p(t["node"], C.c_int32), _p(reward, C.c_double), _p(term, C.c_uint8), _p(trunc, C.c_uint8), _p(t["gather"], C.c_int32),
                _p(t["scatter"], C.c_int32), _p(t["root"], C.c_int32), _p(t["actions"], C.c_int32), _p(out["action"], C.c_int32),
                _p(out["value"], C.c_double), _p(out["upper"], C.c_double), _p(out["sequence"], C.c_int32), _p(out["expanded"], C.c_int32))))

        for x in range(X):
            kernel(x)
            if x == 0:
                tree.fork_device(self, 1, t["root"])
                work.fork_device(self, n, None)
            else:
                work.fork_device(tree, 1, t["gather"])
            _, r, te, tr, _ = work.sim.step(t["actions"].reshape(E * n, 1))
            reward[:], term[:], trunc[:] = r[:, 0], te, tr
            tree.fork_device(work, 1, t["scatter"])
        kernel(X)
        return out
