"""TEST INFRASTRUCTURE ONLY: run the product's kernel source on the CPU (tests/emu/hip_emu.h).

``EmuEngine`` has the Python surface of ``highwayenv_amd.engine.Engine`` so that the parity tests can be written once and run
against the CPU emulation here (no GPU in the build container) and against the real HIP engine on the MI355X (``-m gpu``).  It is
ONE class, built the way ``hwy_create`` / ``with_family`` (hwy_engine.hip) build an engine: ``family_of`` picks the simulation's
driver (IDM with meta-actions on every scenario, the Linear traffic family, direct ego control), a Lidar observation is traced
behind every step / reset / observe like ``launch_stage`` does, and the add-on units -- the TTC grid and planner, fork and score,
OPD, the action mask -- are methods that validate through the product's own ``*_validate`` and then launch through the product's own
launch layer (csrc/hwy_launch_units.h).  Every kernel unit is a library of its own (``UNITS``), so that a mutant of one unit
recompiles that unit's headers only.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from highwayenv_amd import _abi, build as build_flags

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
# HWY_EMU_FLAGS: extra g++ flags for the emulator build (its own library file), e.g. "-ffp-contract=fast -mfma" -- how the test
# suite's tolerances were tried against fused multiply-adds before the kernel build's -ffp-contract=off was put up for an A/B
# (profiles/r03_history.md).  Since the kernel build contracts (build.FP_CONTRACT = "on") the knob runs the other way:
# "-ffp-contract=off" is the strict emulator of tests/test_strict_arithmetic.py.  Every emulator library honours it, each in a file
# named after the flags.
_EXTRA = os.environ.get("HWY_EMU_FLAGS", "").split()


def flagged(out_lib: str) -> str:
    """The file an emulator library built under HWY_EMU_FLAGS goes to: never the file of the default build."""
    if not _EXTRA:
        return out_lib
    return "%s_%08x.so" % (out_lib[:-3], __import__("zlib").crc32(" ".join(_EXTRA).encode()) & 0xffffffff)


def compile_emulator(src_cpp: str, out_lib: str, extra=()) -> None:
    """One emulator library from `src_cpp` (a driver of this tree, or of a mutated copy: tests/mutation_util.py)."""
    # like the kernel build (build.FP_CONTRACT).  "on" = contraction by source expression is a FRONT-END rule: the emulator
    # is compiled by the clang the kernels are compiled by (ROCm's), so the same a*b+c fuse here and on the GPU; g++ 11
    # treats -ffp-contract=on as off and is only the fallback (then: fuse where it likes, same tolerances).
    clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    cxx = "g++"
    if build_flags.FP_CONTRACT == "off":
        contract = ["-ffp-contract=off"]
    elif build_flags.FP_CONTRACT == "on" and os.path.exists(clang):
        cxx, contract = clang, ["-ffp-contract=on", "-mfma"]
    else:
        contract = ["-ffp-contract=fast", "-mfma"]
    tmp = f"{out_lib}.{os.getpid()}.tmp"   # pytest-xdist workers may build at once: never expose a half-written library
    subprocess.run([cxx, "-std=c++20", "-O1", "-pthread", "-fPIC", "-shared", *contract, *extra, "-o", tmp, src_cpp],
                   check=True, capture_output=True)
    os.replace(tmp, out_lib)


class _OpdTree(C.Structure):  # hwy_opd.h: OpdTree
    _fields_ = [(k, C.c_void_p) for k in ("ret", "disc", "upper0", "done", "node", "gather", "scatter", "root", "actions", "created",
                                          "child_mask")]


class _OpdPlan(C.Structure):  # hwy_opd.h: OpdPlan
    _fields_ = [(k, C.c_void_p) for k in ("action", "value", "upper", "sequence", "expanded")]


class _View(C.Structure):  # emu_fork.h: emu_engine_view
    _fields_ = [("cfg", C.POINTER(_abi.HwyConfig)), ("st", C.POINTER(_abi.HwyState)), ("extra", C.POINTER(C.c_double)),
                ("done", C.POINTER(C.c_uint8)), ("episode", C.POINTER(C.c_uint32))]


# The emulator libraries, one per kernel unit: driver source and its own headers (tests/emu), the product headers it is built from
# (csrc; with the driver: what makes a build stale), the environment variable naming a prebuilt (mutated) library instead, the
# (symbol, ctypes struct whose size it must return) checks of a load, and the prefix of its last_error symbol (None: none).
_STEP = ["hwy_device.h", "hwy_wave.h", "hwy_math.h", "hwy_params.h", "hwy_launch_family.h"]
UNITS = {
    "sim": (["emu_engine.cpp", "emu_straight.h"], _STEP + ["hwy_wave2.h", "hwy_net.h", "hwy_ix.h", "hwy_launch_rules.h"], "HWY_EMU_LIB",
            [("emu_config_size", _abi.HwyConfig)], None),
    "traffic": (["emu_traffic.cpp", "emu_straight.h"], _STEP, "HWY_EMU_TRAFFIC_LIB", [("emu_traffic_config_size", _abi.HwyConfig)], None),
    "control": (["emu_control.cpp", "emu_straight.h"], _STEP, "HWY_EMU_CONTROL_LIB", [("emu_control_config_size", _abi.HwyConfig)], None),
    "lidar": (["emu_lidar.cpp"], ["hwy_lidar.h", "hwy_device.h", "hwy_math.h", "hwy_launch_units.h"], "HWY_EMU_LIDAR_LIB",
              [("emu_lidar_config_size", _abi.HwyConfig)], None),
    "ttc": (["emu_ttc.cpp"], ["hwy_ttc.h", "hwy_device.h", "hwy_math.h", "hwy_launch_units.h"], "HWY_EMU_TTC_LIB",
            [("emu_ttc_config_size", _abi.HwyConfig), ("emu_ttc_params_size", _abi.HwyTtcParams)], "emu_ttc"),
    "lookahead": (["emu_lookahead.cpp", "emu_fork.h"], ["hwy_lookahead.h", "hwy_launch_units.h"], "HWY_EMU_LOOKAHEAD_LIB",
                  [("emu_lookahead_config_size", _abi.HwyConfig)], "emu_lookahead"),
    "opd": (["emu_opd.cpp", "emu_fork.h"], ["hwy_opd.h", "hwy_lookahead.h", "hwy_launch_units.h"], "HWY_EMU_OPD_LIB",
            [("emu_opd_config_size", _abi.HwyConfig), ("emu_opd_params_size", _abi.HwyOpdParams), ("emu_opd_tree_size", (_OpdTree, _OpdPlan))],
            "emu_opd"),
    "mask": (["emu_mask.cpp"], ["hwy_mask.h", "hwy_device.h", "hwy_math.h", "hwy_ix.h", "hwy_net.h", "hwy_wave.h", "hwy_launch_units.h"],
             "HWY_EMU_MASK_LIB", [("emu_mask_config_size", _abi.HwyConfig)], "emu_mask"),
}
_libs = {}


def build(unit: str = "sim", force: bool = False) -> str:
    own, headers, env, _, _ = UNITS[unit]
    if os.environ.get(env):
        return os.environ[env]
    name = "libhwy_emu.so" if unit == "sim" else f"libhwy_emu_{unit}.so"
    out = flagged(os.path.join(_HERE, "_build", name))
    srcs = [os.path.join(_HERE, f) for f in own + ["hip_emu.h"]] + [os.path.join(_ROOT, "highwayenv_amd", "csrc", f) for f in headers] + [
        os.path.join(_ROOT, "include", "hwy_engine.h")]
    if force or not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        compile_emulator(srcs[0], out, _EXTRA)
    return out


def build_all() -> None:
    """The suite's own emulator builds (a mutation test: before two processes could both start one)."""
    for unit in UNITS:
        build(unit)


def load(unit: str, path: str):
    """The library of `unit` at `path` (the suite's own, or a mutated build), its struct sizes checked against _abi."""
    L = C.CDLL(path)
    for symbol, structs in UNITS[unit][3]:
        getattr(L, symbol).restype = C.c_size_t
        assert getattr(L, symbol)() == sum(C.sizeof(s) for s in (structs if isinstance(structs, tuple) else (structs,))), symbol
    if UNITS[unit][4]:
        getattr(L, UNITS[unit][4] + "_last_error").restype = C.c_char_p
    if unit == "opd":
        assert L.emu_opd_max_nodes() == _abi.HWY_OPD_MAX_NODES
    return L


def lib(unit: str = "sim"):
    if unit not in _libs:
        _libs[unit] = load(unit, build(unit))
    return _libs[unit]


def last_error(unit: str, L=None) -> str:
    return getattr(L or lib(unit), UNITS[unit][4] + "_last_error")().decode()


def _check(unit: str, rc: int, L=None):
    """Raise what the product's Engine raises for a status (engine.py: _check_scope)."""
    if rc == _abi.HWY_ERR_UNSUPPORTED:
        raise NotImplementedError(last_error(unit, L))
    if rc != 0:
        from highwayenv_amd.engine import EngineError
        raise EngineError(f"status {rc}: {last_error(unit, L)}")


def _p(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def _host_state(st: dict) -> dict:
    return {k: np.ascontiguousarray(st[k]) for k in _abi.STATE_F64 + _abi.STATE_I32 + ["time"]}


# schedule policies of the emulator (hip_emu.h, emu_set_schedule).  wave: "rr" (the default round-robin) or the order in which
# the wavefronts of a workgroup run ahead to the next workgroup barrier, one at a time; lane: the order of the fibers of a
# wavefront between two rendezvous; block: the order of the workgroups of a launch.  "seeded" orders are drawn again at every
# barrier (wave, lane) or launch (block) from the seed.
WAVE_ORDERS = {"rr": 0, "asc": 1, "desc": 2, "seeded": 3}
ORDERS = {"asc": 0, "desc": 2, "seeded": 3}


def schedule_policy(wave="rr", lane="asc", block="asc") -> int:
    return WAVE_ORDERS[wave] | ORDERS[lane] << 4 | ORDERS[block] << 8


class Scheduled:
    """The schedule an emulated engine's launches run under -- the simulation's and the units' alike --, and the rendezvous
    violations they met (schedule_errors: a workgroup barrier or a wave rendezvous whose fibers came from different call sites, a
    block whose threads passed different numbers of barriers, a launch in which no fiber could run any more).  A library's schedule
    is set around each call into it and put back to the default after it, so engines with different schedules can be used side by
    side."""
    _policy = _seed = _calls = _errors = 0
    _error_text = ""

    def set_schedule(self, wave="rr", lane="asc", block="asc", seed=0):
        self._policy, self._seed = schedule_policy(wave, lane, block), int(seed)

    def schedule_errors(self) -> int:
        return self._errors

    def schedule_error_text(self) -> str:
        return self._error_text

    def _scheduled(self, L, call):
        L.emu_schedule_errors.restype = C.c_longlong
        L.emu_clear_schedule_errors()
        # every launch of a seeded schedule draws from its own stream
        L.emu_set_schedule(C.c_int(self._policy), C.c_uint64((self._seed * 0x9E3779B1 + self._calls) & (2 ** 64 - 1)))
        self._calls += 1
        try:
            return call()
        finally:
            n = L.emu_schedule_errors()
            if n:
                if not self._errors:
                    buf = C.create_string_buffer(4096)
                    L.emu_schedule_error_text(buf, C.c_int(len(buf)))
                    self._error_text = buf.value.decode()
                self._errors += n
            L.emu_set_schedule(C.c_int(0), C.c_uint64(0))
            L.emu_clear_schedule_errors()


def _run(sched, L, call):
    return call() if sched is None else sched._scheduled(L, call)


# ---- the add-on units on a host state ([E, N] arrays of a get_state); `sched`: a Scheduled whose schedule the launch runs under ----
def trace(cfg: _abi.HwyConfig, st: dict, sched=None) -> np.ndarray:
    """The lidar kernel (hwy_lidar.h): obs f32 [E, A, cells, 2]."""
    assert cfg.obs_type == _abi.OBS_LIDAR
    s = _abi.state_struct(_host_state(st))
    obs = np.full((cfg.num_envs, cfg.num_agents, cfg.lidar_cells, 2), np.nan, np.float32)
    assert _run(sched, lib("lidar"), lambda: lib("lidar").emu_lidar_observe(C.byref(cfg), C.byref(s), _p(obs, C.c_float))) == 0
    return obs


def ttc_shape(cfg: _abi.HwyConfig, params: _abi.HwyTtcParams) -> tuple:
    return (cfg.num_target_speeds, cfg.lanes_count, params.time_steps)


def ttc_status(cfg: _abi.HwyConfig, params) -> int:
    """The status the entry points return for (config, params) before any launch (csrc/hwy_ttc.h: ttc_validate)."""
    return lib("ttc").emu_ttc_validate(C.byref(cfg), None if params is None else C.byref(params))


def mdp_plan(cfg: _abi.HwyConfig, st: dict, params: _abi.HwyTtcParams, return_q=False, return_grid=False, sched=None, plan=True):
    """hwy_mdp_plan (plan=False: hwy_ttc_grid) on a host state: (action int32 [E, A], q f64 [E, A, 5], grid f32 [E, A, V, L, T])."""
    s = _abi.state_struct(_host_state(st))
    _check("ttc", ttc_status(cfg, params))  # (first: the shape of the outputs needs valid params)
    rows = (cfg.num_envs, cfg.num_agents)
    action = np.full(rows, -1, np.int32) if plan else None
    q = np.full((*rows, 5), np.nan, np.float64) if return_q else None
    grid = np.full((*rows, *ttc_shape(cfg, params)), np.nan, np.float32) if return_grid else None
    _check("ttc", _run(sched, lib("ttc"), lambda: lib("ttc").emu_ttc_launch(
        C.byref(cfg), C.byref(s), C.byref(params), int(plan), _p(grid, C.c_float), _p(action, C.c_int32), _p(q, C.c_double))))
    return action, q, grid


def ttc_grid(cfg: _abi.HwyConfig, st: dict, params: _abi.HwyTtcParams, sched=None) -> np.ndarray:
    return mdp_plan(cfg, st, params, return_grid=True, sched=sched, plan=False)[2]


def fork_status(dst_cfg, src_cfg, same_engine=False, branches=1, has_source=False) -> int:
    """The status hwy_fork_device returns for two configs before any launch (csrc/hwy_lookahead.h: fork_validate)."""
    return lib("lookahead").emu_lookahead_fork_status(C.byref(dst_cfg), C.byref(src_cfg), int(same_engine), int(branches), int(has_source))


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
    L = lib("lookahead")
    _check("lookahead", L.emu_lookahead_score_status(
        C.byref(cfg), C.c_int32(K), C.c_int32(B), C.c_double(gamma), int(first is not None),
        int(rew is not None and term is not None and trunc is not None), int(out["q"] is not None), int(out["best_action"] is not None)))
    _check("lookahead", _run(sched, L, lambda: L.emu_lookahead_score(
        C.byref(cfg), C.c_int32(K), C.c_int32(B), C.c_double(gamma), _p(first, C.c_int32), _p(rew, C.c_double), _p(term, C.c_uint8),
        _p(trunc, C.c_uint8), _p(out["returns"], C.c_double), _p(out["q"], C.c_double), _p(out["best_action"], C.c_int32),
        _p(out["best_branch"], C.c_int32))))
    return out


def opd_validate(src_cfg, tree_cfg, work_cfg, params, has_action=True) -> int:
    """The status hwy_opd_plan_device returns before any launch (csrc/hwy_opd.h: opd_validate); the reason: ``last_error("opd")``."""
    return lib("opd").emu_opd_validate(C.byref(src_cfg), C.byref(tree_cfg), C.byref(work_cfg), None if params is None else C.byref(params),
                                       int(has_action))


def opd_sequence(n: int, expansions: int, masked: bool) -> list:
    """The operations hwy_opd.h's opd_expand -- the sequence of hwy_opd_plan_device -- runs, in order, as words."""
    buf = C.create_string_buffer(1 << 16)
    assert lib("opd").emu_opd_sequence(C.c_int32(n), C.c_int32(expansions), int(masked), buf, C.c_int(len(buf))) == 0
    return buf.value.decode().split()


def mask_status(cfg: _abi.HwyConfig, L=None) -> int:
    """The status the entry points return for a config before any launch (csrc/hwy_mask.h: mask_validate)."""
    return (L or lib("mask")).emu_mask_validate(C.byref(cfg))


def action_mask(cfg: _abi.HwyConfig, st: dict, L=None, sched=None) -> np.ndarray:
    """The mask kernel (hwy_mask.h) on a host state: bool [E, A, n_ids].  `L`: another (mutated) library."""
    L = L or lib("mask")
    s = _abi.state_struct(_host_state(st))
    _check("mask", mask_status(cfg, L), L)
    mask = np.full((cfg.num_envs, cfg.num_agents, L.emu_mask_num_ids(C.byref(cfg))), 255, np.uint8)
    _check("mask", _run(sched, L, lambda: L.emu_mask_launch(C.byref(cfg), C.byref(s), C.c_int(cfg.num_vehicles), _p(mask, C.c_uint8))), L)
    assert ((mask == 0) | (mask == 1)).all(), "the kernel left a byte unwritten"
    return mask.astype(bool)


# ---- the engine ------------------------------------------------------------------------------------------------------------------------
def family_of(cfg: _abi.HwyConfig) -> str:
    """The unit whose driver simulates a config, as hwy_engine.hip's with_family picks the kernel family: the scenario first (the
    intersection and the road networks run IDM traffic with meta-actions), then Linear traffic, then direct ego control."""
    if cfg.scenario == _abi.SCENARIO_HIGHWAY and cfg.traffic_model == _abi.TRAFFIC_LINEAR:
        return "traffic"
    if cfg.scenario == _abi.SCENARIO_HIGHWAY and cfg.ego_control == _abi.EGO_DIRECT:
        return "control"
    return "sim"


class EmuEngine(Scheduled):
    #: another (mutated) library of the OPD unit for this engine's plans (tests/test_mask_mutations.py)
    opd_lib = None

    def __init__(self, cfg: _abi.HwyConfig):
        self.cfg = cfg
        self.E, self.N, self.A = cfg.num_envs, cfg.num_vehicles, cfg.num_agents
        self.family = family_of(cfg)
        self.ix = cfg.scenario == _abi.SCENARIO_INTERSECTION
        self.lidar = cfg.obs_type == _abi.OBS_LIDAR
        # what the step kernels of a Lidar engine see (hwy_params.h: params_from_config): they run WITHOUT the observation -- a
        # one-column Kinematics observation stands in for the null pointer, nothing of the state depends on it -- and hwy_lidar.h's
        # kernel traces the state each call left behind (hwy_engine.hip: launch_stage)
        self.sim_cfg = cfg
        if self.lidar:
            assert cfg.scenario == _abi.SCENARIO_HIGHWAY
            self.sim_cfg = _abi.HwyConfig.from_buffer_copy(bytes(cfg))
            self.sim_cfg.obs_type = _abi.OBS_KINEMATICS
        self.st = _abi.alloc_state_ix(self.E, self.N) if self.ix else _abi.alloc_state(self.E, self.N)
        self.done = np.zeros(self.E, np.uint8)
        self.episode = np.zeros(self.E, np.uint32)
        self.autoreset = (0, 0, 2.0, 1.0, -1)
        self.extra = None  # the family's extra planes, in the device layout
        if self.family == "traffic":
            self.extra = np.zeros((_abi.HWY_BEHAVIOR_PARAMS, self.E, self.N))  # [k][E][N]
        elif self.family == "control":
            self.extra = np.zeros((2, self.E, self.A))  # acceleration | steering
        if self.ix:  # next-episode pre-warming buffers (hwy_engine.hip allocates the same on the device)
            self.shadow = (np.zeros((9, self.E, self.N)), np.zeros((self.E, self.N), np.int32),
                           np.zeros((self.E, self.N), np.int64), np.full((self.E, 4), -1, np.int32))

    def close(self):
        pass

    def sync(self):
        pass

    # -- state ----------------------------------------------------------------------------------
    def set_state(self, st):
        self.st = {k: np.array(st[k], copy=True) for k in self.st}  # (the planes of hwy_state; a dict may carry a family's extras too)
        self.done[:] = 0

    def get_state(self):
        st = _abi.copy_state(self.st)
        if self.ix:  # like hwy_get_state: the planes of an empty slot (and an impact without its flag) are unspecified: zeros
            absent = (st["flags"] & _abi.F_ABSENT) != 0
            for k in _abi.STATE_F64 + ["lane", "target_lane", "speed_index", "route"]:
                st[k][absent] = 0
            st["flags"][absent] = _abi.F_ABSENT
            no_impact = (st["flags"] & _abi.F_HAS_IMPACT) == 0
            st["impact_x"][no_impact] = 0
            st["impact_y"][no_impact] = 0
        return st

    def set_behavior(self, params):
        a = np.asarray(params, np.float64)
        assert self.family == "traffic" and a.shape == (self.E, self.N, _abi.HWY_BEHAVIOR_PARAMS)
        self.extra = np.ascontiguousarray(a.transpose(2, 0, 1))

    def get_behavior(self):
        assert self.family == "traffic"
        return np.ascontiguousarray(self.extra.transpose(1, 2, 0))

    def set_controls(self, acceleration, steering):
        assert self.family == "control"
        self.extra = np.ascontiguousarray(np.stack([np.asarray(acceleration, np.float64).reshape(self.E, self.A),
                                                    np.asarray(steering, np.float64).reshape(self.E, self.A)]))

    def get_controls(self):
        assert self.family == "control"
        return self.extra[0].copy(), self.extra[1].copy()

    def set_autoreset(self, enabled, base_seed=0, ego_spacing=2.0, vehicles_density=1.0, initial_lane_id=-1):
        if self.ix and int(base_seed) != self.autoreset[1]:
            self.shadow[3][...] = -1
        self.autoreset = (int(enabled), int(base_seed), float(ego_spacing), float(vehicles_density), int(initial_lane_id))

    def set_block_order(self, env_of_block=None):
        self._block_env = None if env_of_block is None else np.ascontiguousarray(env_of_block, np.uint16)

    # -- the simulation's driver ------------------------------------------------------------------
    def _driver(self, name, head, tail, rollout=0):
        """One call of the family's driver (emu_engine.cpp / emu_traffic.cpp / emu_control.cpp over emu_straight.h).  The IDM driver
        takes what only it has -- the intersection's shadow planes, the block order, a multi-step launch -- through setters."""
        L = lib(self.family)
        if self.family != "sim":
            call = lambda: getattr(L, f"emu_{self.family}_{name}")(*head, _p(self.extra, C.c_double), *tail)  # noqa: E731
        else:
            L.emu_set_shadow(*([_p(a, t) for a, t in zip(self.shadow, (C.c_double, C.c_int32, C.c_int64, C.c_int32))] if self.ix
                               else [None] * 4))
            be = getattr(self, "_block_env", None)
            L.emu_set_block_order(None if be is None else be.ctypes.data_as(C.c_void_p))
            L.emu_set_rollout(C.c_int(rollout))
            call = lambda: getattr(L, f"emu_{name}")(*head, *tail)  # noqa: E731
        try:
            assert self._scheduled(L, call) == 0
        finally:
            if self.family == "sim":
                L.emu_set_rollout(C.c_int(0))

    def _run(self, mode, n_frames, actions, k_steps=0):
        """mode: emu_straight.h (0 = frames only, 1 = full policy steps, 2 = observe); outputs with a leading axis of max(k_steps, 1)."""
        E, A, K, c = self.E, self.A, max(k_steps, 1), self.sim_cfg
        acts = None if actions is None else np.ascontiguousarray(np.asarray(actions, np.int32).reshape(K, E, A))
        obs = np.zeros((K, E, A, *_abi.obs_shape(c)), np.float32)
        reward = np.zeros((K, E, A))
        term, trunc = np.zeros((K, E), np.uint8), np.zeros((K, E), np.uint8)
        speed, crashed = np.zeros((K, E, A)), np.zeros((K, E, A), np.uint8)
        s, ar = _abi.state_struct(self.st), self.autoreset
        steps = () if self.family == "sim" else (C.c_int(k_steps),)
        self._driver("run", (C.byref(c), C.byref(s)),
                     (_p(self.done, C.c_uint8), _p(self.episode, C.c_uint32), C.c_int(mode), C.c_int(n_frames), *steps, _p(acts, C.c_int32),
                      _p(obs, C.c_float), _p(reward, C.c_double), _p(term, C.c_uint8), _p(trunc, C.c_uint8), _p(speed, C.c_double),
                      _p(crashed, C.c_uint8), C.c_int(ar[0]), C.c_uint64(ar[1]), C.c_double(ar[2]), C.c_double(ar[3]), C.c_int(ar[4])),
                     rollout=k_steps)
        return obs, reward, term.astype(bool), trunc.astype(bool), {"speed": speed, "crashed": (crashed & 1).astype(bool),
                                                                    "arrived": (crashed & 2).astype(bool)}

    def _check_actions(self, actions):
        a = np.asarray(actions)
        if ((a < 0) | (a >= (3 if self.ix else _abi.num_actions(self.cfg)))).any():  # hwy_step: HWY_ERR_ACTION
            if self.family == "control":
                raise IndexError("action id outside the throttle x steering table")
            raise KeyError("invalid meta-action")

    # -- stepping -----------------------------------------------------------------------------------
    def step_frames(self, actions, n_frames):
        self._run(0, n_frames, actions)

    def step(self, actions):
        self._check_actions(actions)
        obs, reward, term, trunc, info = self._run(1, self.cfg.frames_per_step, actions)
        return (self.observe() if self.lidar else obs[0]), reward[0], term[0], trunc[0], {k: v[0] for k, v in info.items()}

    def observe(self):
        return trace(self.cfg, self.st, self) if self.lidar else self._run(2, 0, None)[0][0]

    def rollout(self, actions):
        """hwy_rollout_device: actions [K, E, A] -> (obs [K, E, A, ...], reward [K, E, A], terminated [K, E], truncated [K, E],
        info) -- ONE multi-step launch; on a Lidar engine K x (step + trace)."""
        acts = np.ascontiguousarray(np.asarray(actions, np.int32).reshape(-1, self.E, self.A))
        if not self.lidar:
            return self._run(1, self.cfg.frames_per_step, acts, k_steps=acts.shape[0])
        outs = [self.step(a) for a in acts]
        info = {key: np.stack([o[4][key] for o in outs]) for key in outs[0][4]}
        return tuple(np.stack([o[j] for o in outs]) for j in range(4)) + (info,)

    def reset(self, seeds=None, mask=None, ego_spacing=2.0, vehicles_density=1.0, initial_lane_id=-1, base_seed=0):
        obs = np.zeros((self.E, self.A, *_abi.obs_shape(self.sim_cfg)), np.float32)
        sd = None if seeds is None else np.ascontiguousarray(seeds, np.uint64)
        mk = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        s = _abi.state_struct(self.st)
        self._driver("reset", (C.byref(self.sim_cfg), C.byref(s)),
                     (_p(self.done, C.c_uint8), _p(self.episode, C.c_uint32), _p(mk, C.c_uint8), _p(sd, C.c_uint64), C.c_uint64(base_seed),
                      C.c_double(ego_spacing), C.c_double(vehicles_density), C.c_int(initial_lane_id), _p(obs, C.c_float)))
        if self.lidar:
            obs = self.observe()
            if mask is not None:  # hwy_reset: rows of unmasked environments are left untouched (zeros from Engine.reset)
                obs[np.asarray(mask) == 0] = 0
        return obs

    def debug_math(self, op, x):
        xin = np.ascontiguousarray(x, np.float64).ravel()
        out = np.empty_like(xin)
        getattr(lib(self.family), "emu_debug_math" if self.family == "sim" else f"emu_{self.family}_debug_math")(
            C.c_int(op), _p(xin, C.c_double), _p(out, C.c_double), C.c_longlong(xin.size))
        return out.reshape(np.shape(x))

    # -- time-to-collision grid and finite-MDP planner (csrc/hwy_ttc.h) ---------------------------------
    def ttc_shape(self, params):
        return ttc_shape(self.cfg, params)

    def ttc_grid(self, params):
        return ttc_grid(self.cfg, self.get_state(), params, self)

    def mdp_plan(self, params, return_q=False, return_grid=False):
        return mdp_plan(self.cfg, self.get_state(), params, return_q, return_grid, self)

    # -- environment fork and scoring of action sequences (csrc/hwy_lookahead.h) -------------------------
    def _view(self):
        """emu_fork.h's view of this engine's arrays, and what has to stay alive while it is used."""
        s = _abi.state_struct(self.st)
        return _View(C.pointer(self.cfg), C.pointer(s), _p(self.extra, C.c_double), _p(self.done, C.c_uint8), _p(self.episode, C.c_uint32)), s

    def _fork(self, src, branches, idx, host_indices):
        L = lib("lookahead")
        _check("lookahead", fork_status(self.cfg, src.cfg, self is src, branches, idx is not None))
        (d, _d), (s, _s) = self._view(), src._view()
        _check("lookahead", self._scheduled(L, lambda: L.emu_lookahead_fork(C.byref(d), C.byref(s), C.c_int32(int(branches)),
                                                                            _p(idx, C.c_int32), int(host_indices))))

    def fork_from(self, src: "EmuEngine", branches: int = 1, source=None):
        idx = None
        if source is not None:
            idx = np.ascontiguousarray(source, dtype=np.int32)
            if idx.shape != (self.E,):
                raise ValueError(f"fork: source has shape {idx.shape}, this engine needs ({self.E},)")
        self._fork(src, branches, idx, True)

    fork = fork_from

    def fork_device(self, src: "EmuEngine", branches: int = 1, source=None):
        """hwy_fork_device: ``source`` int32 [E] stands for the device array of indices (not validated), None for j // branches."""
        idx = None if source is None else np.ascontiguousarray(source, dtype=np.int32)
        assert idx is None or idx.shape == (self.E,)
        self._fork(src, branches, idx, False)

    def score(self, k_steps, branches, gamma, first_action, reward, terminated, truncated, **kw):
        return score(self.cfg, k_steps, branches, gamma, first_action, reward, terminated, truncated, sched=self, **kw)

    def score_rollout(self, actions, branches: int, gamma: float = 1.0) -> dict:
        acts = np.ascontiguousarray(np.asarray(actions, np.int32).reshape(-1, self.E, self.A))
        K, A, B = acts.shape[0], self.A, int(branches)
        if B < 1 or self.E % B:
            raise ValueError(f"score_rollout: branches={B} does not divide the engine's {self.E} environments")
        if ((acts < 0) | (acts >= _abi.num_actions(self.cfg))).any():  # hwy_score_rollout: HWY_ERR_ACTION
            raise (IndexError if self.cfg.ego_control == _abi.EGO_DIRECT else KeyError)("action id out of range")
        _, reward, term, trunc, _ = self._run(1, self.cfg.frames_per_step, acts, k_steps=K)
        want = ("returns", "q", "best_action", "best_branch") if A == 1 else ("returns", "best_branch")
        out = self.score(K, B, gamma, acts[0] if A == 1 else None, reward, term, trunc, want=want)
        out.update(reward=reward, terminated=term, truncated=trunc)
        return out

    # -- optimistic planning, one tree per environment (csrc/hwy_opd.h) -----------------------------------
    def opd_plan(self, tree: "EmuEngine", work: "EmuEngine", params: _abi.HwyOpdParams) -> dict:
        """hwy_opd_plan: the validation, then ONE call of the OPD unit that runs the product's sequence (hwy_opd.h: opd_expand) --
        the tree kernels and the forks in that library, the work engine's mask and step called back from it.  ``last_tree``: the
        planner's arrays of the last plan (for the tests: which nodes were created)."""
        _check("opd", opd_validate(self.cfg, tree.cfg, work.cfg, params))
        if tree is self or work is self or tree is work:
            raise ValueError("src, tree and work must be three engines")
        if tree.autoreset[0] or work.autoreset[0]:
            raise ValueError("tree and work must run with auto-reset off")
        return self._opd_launch(tree, work, params)

    def _opd_launch(self, tree, work, params, without=()):
        """The launches behind a passed validation.  ``last_tree`` / ``last_plan`` are set before them; `without`: arrays of the
        tree handed over as NULL (tests/test_unit_launch_layer.py: what the launch rule refuses)."""
        L = self.opd_lib or lib("opd")
        E, n, M = self.E, params.n_ids, params.nodes
        X = params.budget // n
        t = {"ret": np.full((E, M), np.nan), "disc": np.full((E, M), np.nan), "upper0": np.full((E, M), np.nan),
             "done": np.full((E, M), 0xff, np.uint8), "node": np.full((E, X), -7, np.int32), "gather": np.full(E * n, -7, np.int32),
             "scatter": np.full(E * M, -7, np.int32), "root": np.full(E * M, -7, np.int32), "actions": np.full(E * n, -7, np.int32),
             "created": np.full((E, M), 0xff, np.uint8), "child_mask": np.full((E * n, n), 0xff, np.uint8)}
        reward, term, trunc = np.full(E * n, np.nan), np.zeros(E * n, np.uint8), np.zeros(E * n, np.uint8)
        out = {"action": np.full(E, -7, np.int32), "value": np.full(E, np.nan), "upper": np.full(E, np.nan),
               "sequence": np.full((E, X), -7, np.int32), "expanded": np.full(E, -7, np.int32)}
        self.last_tree, self.last_plan, raised = t, out, []

        def callback(fn):
            def guarded():
                try:
                    fn()
                    return 0
                except BaseException as e:  # (an exception cannot cross the C frames)
                    raised.append(e)
                    return _abi.HWY_ERR_INVALID_ARG
            return C.CFUNCTYPE(C.c_int)(guarded)

        def mask():
            t["child_mask"][...] = work.action_mask()[:, 0]

        def step():  # hwy_step_device: no validation of the action ids, no copy of the observation
            _, r, te, tr, _ = work._run(1, work.cfg.frames_per_step, t["actions"])
            reward[:], term[:], trunc[:] = r[0, :, 0], te[0], tr[0]

        views = [e._view() for e in (self, tree, work)]
        rc = self._scheduled(L, lambda: L.emu_opd_plan(
            *(C.byref(v) for v, _ in views), C.byref(params), C.byref(_OpdTree(*(None if k in without else t[k].ctypes.data for k, _ in _OpdTree._fields_))),
            _p(reward, C.c_double), _p(term, C.c_uint8), _p(trunc, C.c_uint8),
            C.byref(_OpdPlan(*(out[k].ctypes.data for k, _ in _OpdPlan._fields_))), callback(mask), callback(step)))
        if raised:
            raise raised[0]
        _check("opd", rc, L)
        return out

    # -- action mask (csrc/hwy_mask.h) ---------------------------------------------------------------------
    def action_mask(self) -> np.ndarray:
        return action_mask(self.cfg, self.get_state(), sched=self)


def force_block_kernel(on: bool):
    """Use the generic workgroup kernel even for N <= 64 (the engine's HWY_STEP_KERNEL=block)."""
    lib().emu_force_block_kernel(C.c_int(int(on)))


def philox_uniform2(seed, vehicle, episode, draw):
    u0, u1 = C.c_double(), C.c_double()
    lib().emu_philox_uniform2(C.c_uint64(seed), C.c_uint32(vehicle), C.c_uint32(episode), C.c_uint32(draw),
                              C.byref(u0), C.byref(u1))
    return u0.value, u1.value


def behavior_draw(seed: int, vehicle: int, episode: int) -> np.ndarray:
    """The device's Philox draw of one Linear vehicle's parameters (hwy_device.h: linear_behavior_draw)."""
    out = np.zeros(_abi.HWY_BEHAVIOR_PARAMS)
    lib("traffic").emu_traffic_behavior_draw(C.c_uint64(seed), C.c_int(vehicle), C.c_uint32(episode), _p(out, C.c_double))
    return out
