"""TEST INFRASTRUCTURE ONLY: the masked tree kernel of the optimistic planner on the CPU (tests/emu/emu_opd_mask.cpp).

``EmuOpdMaskEngine`` is ``EmuOpdEngine`` plus ``action_mask`` (tests/emu/emu_mask.py) and an ``opd_plan`` that honours
``HWY_OPD_MASKED`` in ``params.flags``: per expansion what ``hwy_opd_plan_device`` enqueues then -- ``hwy_opd_masked_kernel``, the
gather tree -> work, the mask kernel on the work engine, one step of it, the scatter work -> tree -- and one more kernel launch for
the plan.  Without the flag it is ``EmuOpdEngine.opd_plan``.  ``HWY_EMU_OPD_MASK_LIB`` names a prebuilt (mutated) library instead
(tests/test_mask_mutations.py)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from highwayenv_amd import _abi

from . import emu, emu_mask, emu_opd
from .emu import _p
from .emu_opd import EmuOpdEngine

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_lib = None


def build(force: bool = False) -> str:
    if os.environ.get("HWY_EMU_OPD_MASK_LIB"):
        return os.environ["HWY_EMU_OPD_MASK_LIB"]
    out = emu.flagged(os.path.join(_HERE, "_build", "libhwy_emu_opd_mask.so"))
    srcs = [os.path.join(_HERE, f) for f in ("emu_opd_mask.cpp", "hip_emu.h")] + [
        os.path.join(_ROOT, "highwayenv_amd", "csrc", f) for f in ("hwy_opd.h", "hwy_lookahead.h")] + [
        os.path.join(_ROOT, "include", "hwy_engine.h")]
    if force or not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        emu.compile_emulator(srcs[0], out, emu._EXTRA)
    return out


def load(path: str):
    L = C.CDLL(path)
    L.emu_opd_mask_params_size.restype = C.c_size_t
    L.emu_opd_mask_last_error.restype = C.c_char_p
    assert L.emu_opd_mask_params_size() == C.sizeof(_abi.HwyOpdParams)
    return L


def lib():
    global _lib
    if _lib is None:
        _lib = load(build())
    return _lib


class EmuOpdMaskEngine(EmuOpdEngine):
    #: another (mutated) library of the masked kernel for this engine's plans (tests/test_mask_mutations.py)
    masked_lib = None

    def action_mask(self) -> np.ndarray:
        return emu_mask.action_mask(self.cfg, self.get_state())

    def opd_plan(self, tree, work, params: _abi.HwyOpdParams) -> dict:
        emu_opd._check(emu_opd.validate(self.cfg, tree.cfg, work.cfg, params))
        if not params.flags & _abi.HWY_OPD_MASKED:
            return super().opd_plan(tree, work, params)
        if tree is self or work is self or tree is work:
            raise ValueError("src, tree and work must be three engines")
        L = self.masked_lib or lib()
        E, n, M = self.E, params.n_ids, params.nodes
        X = params.budget // n
        t = {"ret": np.full((E, M), np.nan), "disc": np.full((E, M), np.nan), "upper0": np.full((E, M), np.nan),
             "done": np.full((E, M), 0xff, np.uint8), "node": np.full((E, X), -7, np.int32), "gather": np.full(E * n, -7, np.int32),
             "scatter": np.full(E * M, -7, np.int32), "root": np.full(E * M, -7, np.int32), "actions": np.full(E * n, -7, np.int32),
             "created": np.full((E, M), 0xff, np.uint8), "child_mask": np.full((E * n, n), 0xff, np.uint8)}
        reward, term, trunc = np.full(E * n, np.nan), np.zeros(E * n, np.uint8), np.zeros(E * n, np.uint8)
        out = {"action": np.full(E, -7, np.int32), "value": np.full(E, np.nan), "upper": np.full(E, np.nan),
               "sequence": np.full((E, X), -7, np.int32), "expanded": np.full(E, -7, np.int32)}

        def kernel(x):
            rc = self.sched._scheduled(L, lambda: L.emu_opd_masked_kernel(
                C.c_int32(E), C.c_int32(n), C.c_int32(X), C.c_int32(x), C.c_double(params.gamma), C.c_double(params.bound),
                _p(t["ret"], C.c_double), _p(t["disc"], C.c_double), _p(t["upper0"], C.c_double), _p(t["done"], C.c_uint8),
                _p(t["node"], C.c_int32), _p(reward, C.c_double), _p(term, C.c_uint8), _p(trunc, C.c_uint8), _p(t["gather"], C.c_int32),
                _p(t["scatter"], C.c_int32), _p(t["root"], C.c_int32), _p(t["actions"], C.c_int32), _p(out["action"], C.c_int32),
                _p(out["value"], C.c_double), _p(out["upper"], C.c_double), _p(out["sequence"], C.c_int32), _p(out["expanded"], C.c_int32),
                _p(t["child_mask"], C.c_uint8), _p(t["created"], C.c_uint8)))
            assert rc == 0, L.emu_opd_mask_last_error().decode()

        for x in range(X):
            kernel(x)
            if x == 0:
                tree.fork_device(self, 1, t["root"])
                work.fork_device(self, n, None)
            else:
                work.fork_device(tree, 1, t["gather"])
            t["child_mask"][...] = emu_mask.action_mask(work.cfg, work.get_state())[:, 0]
            _, r, te, tr, _ = work.sim.step(t["actions"].reshape(E * n, 1))
            reward[:], term[:], trunc[:] = r[:, 0], te, tr
            tree.fork_device(work, 1, t["scatter"])
        kernel(X)
        self.last_tree = t   # (for the tests: which nodes were created)
        return out
