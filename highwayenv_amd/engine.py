"""Thin object wrapper over the C-ABI (include/hwy_engine.h): one ``Engine`` == one GPU's
batch of E environments.  Host numpy in / numpy out for the gymnasium-style API, raw device
pointers for on-GPU policies, RCCL gathers and the benchmark.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi, _lib


class EngineError(RuntimeError):
    pass


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class Engine:
    def __init__(self, cfg: _abi.HwyConfig, device: int = 0, stream: int | None = None):
        self._lib = _lib.load()
        self.cfg = cfg
        self.E, self.N, self.A = cfg.num_envs, cfg.num_vehicles, cfg.num_agents
        self.V, self.F = cfg.obs_vehicles, cfg.obs_features
        h = C.c_void_p()
        rc = self._lib.hwy_create(C.byref(cfg), int(device), C.c_void_p(stream or 0), C.byref(h))
        if rc != 0:
            msg = self._lib.hwy_last_error(None).decode()
            raise EngineError(f"hwy_create failed ({self._lib.hwy_status_string(rc).decode()}): {msg}")
        self._h = h
        self.device = device

    # -- lifetime -----------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.hwy_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc == _abi.HWY_ERR_ACTION:
            # the reference raises KeyError from self.actions[int(action)] (envs/common/action.py:260), and IndexError from
            # all_actions[action] of a DiscreteAction (action.py:195; a negative id, which Python would wrap, is rejected too)
            if self.cfg.ego_control == _abi.EGO_DIRECT:
                raise IndexError(self._lib.hwy_last_error(self._h).decode())
            raise KeyError(self._lib.hwy_last_error(self._h).decode())
        if rc != 0:
            raise EngineError(f"{self._lib.hwy_status_string(rc).decode()}: {self._lib.hwy_last_error(self._h).decode()}")

    # -- state --------------------------------------------------------------------------------
    def set_state(self, st: dict):
        """hwy_set_state reads E*N elements per vehicle field and E per env field through raw pointers: every array is
        coerced to its dtype and its shape is checked here, so a dict built for another batch raises instead of
        reading out of bounds."""
        E, N = self.E, self.N
        ix = self.cfg.scenario == _abi.SCENARIO_INTERSECTION
        want = {k: (np.float64, (E, N)) for k in _abi.STATE_F64}
        want.update({k: (np.int32, (E, N)) for k in _abi.STATE_I32})
        want["time"] = (np.float64, (E,))
        if ix:
            want["route"], want["road_steps"] = (np.int64, (E, N)), (np.int32, (E,))
        out = {}
        for k, (dt, shape) in want.items():
            if k not in st:
                raise ValueError(f"set_state: missing field {k!r}")
            a = np.ascontiguousarray(st[k], dtype=dt)
            if a.shape != shape:
                raise ValueError(f"set_state: field {k!r} has shape {a.shape}, this engine needs {shape} "
                                 f"(num_envs={E}, slots per env={N})")
            out[k] = a
        st = out
        s = _abi.state_struct(st)
        self._check(self._lib.hwy_set_state(self._h, C.byref(s)))

    def get_state(self) -> dict:
        ix = self.cfg.scenario == _abi.SCENARIO_INTERSECTION
        st = _abi.alloc_state_ix(self.E, self.N) if ix else _abi.alloc_state(self.E, self.N)
        s = _abi.state_struct(st)
        self._check(self._lib.hwy_get_state(self._h, C.byref(s)))
        return st

    def set_behavior(self, params):
        """hwy_set_behavior: the Linear traffic family's per-vehicle parameters [E, N, 5]
        (ACCELERATION_PARAMETERS[0..2] | STEERING_PARAMETERS[0..2])."""
        a = np.ascontiguousarray(params, dtype=np.float64)
        if a.shape != (self.E, self.N, _abi.HWY_BEHAVIOR_PARAMS):
            raise ValueError(f"set_behavior: shape {a.shape}, this engine needs {(self.E, self.N, _abi.HWY_BEHAVIOR_PARAMS)}")
        self._check(self._lib.hwy_set_behavior(self._h, _ptr(a)))

    def get_behavior(self) -> np.ndarray:
        out = np.empty((self.E, self.N, _abi.HWY_BEHAVIOR_PARAMS), np.float64)
        self._check(self._lib.hwy_get_behavior(self._h, _ptr(out)))
        return out

    def set_controls(self, acceleration, steering):
        """hwy_set_controls: the (acceleration, steering) pair stored on every controlled vehicle of a direct-control engine
        (``Vehicle.action``), [E, A] each."""
        a = np.ascontiguousarray(acceleration, dtype=np.float64)
        s = np.ascontiguousarray(steering, dtype=np.float64)
        if a.shape != (self.E, self.A) or s.shape != (self.E, self.A):
            raise ValueError(f"set_controls: shapes {a.shape}, {s.shape}, this engine needs {(self.E, self.A)}")
        self._check(self._lib.hwy_set_controls(self._h, _ptr(a), _ptr(s)))

    def get_controls(self):
        """(acceleration, steering) [E, A]: the acceleration is what ``Vehicle.clip_actions`` left in the stored action."""
        a, s = np.empty((self.E, self.A), np.float64), np.empty((self.E, self.A), np.float64)
        self._check(self._lib.hwy_get_controls(self._h, _ptr(a), _ptr(s)))
        return a, s

    # -- stepping -----------------------------------------------------------------------------
    def step(self, actions):
        E, A = self.E, self.A
        acts = np.ascontiguousarray(np.asarray(actions, np.int32).reshape(E, A))
        obs = np.empty((E, A, *_abi.obs_shape(self.cfg)), np.float32)
        reward = np.empty((E, A), np.float64)
        term = np.empty(E, np.uint8)
        trunc = np.empty(E, np.uint8)
        speed = np.empty((E, A), np.float64)
        crashed = np.empty((E, A), np.uint8)
        self._check(self._lib.hwy_step(self._h, _ptr(acts), _ptr(obs), _ptr(reward), _ptr(term), _ptr(trunc),
                                       _ptr(speed), _ptr(crashed)))
        # info_crashed: bit 0 = vehicle.crashed; the intersection scenario adds bit 1 = has_arrived(vehicle) (hwy_engine.h)
        return obs, reward, term.astype(bool), trunc.astype(bool), {"speed": speed, "crashed": (crashed & 1).astype(bool),
                                                                    "arrived": (crashed & 2).astype(bool)}

    def step_device(self, d_actions: int, d_obs: int, d_reward: int, d_terminated: int, d_truncated: int,
                    d_info_speed: int = 0, d_info_crashed: int = 0):
        """Enqueue one batched policy step on raw device pointers; does not synchronise."""
        vp = C.c_void_p
        self._check(self._lib.hwy_step_device(self._h, vp(d_actions), vp(d_obs), vp(d_reward), vp(d_terminated),
                                              vp(d_truncated), vp(d_info_speed or None), vp(d_info_crashed or None)))

    def rollout_device(self, k_steps: int, d_actions: int, d_obs: int, d_reward: int, d_terminated: int, d_truncated: int,
                       d_info_speed: int = 0, d_info_crashed: int = 0):
        """Enqueue ``k_steps`` consecutive policy steps with pre-staged actions (hwy_rollout_device: block k of every plane
        belongs to step k; ONE launch on the one-wavefront kernel); does not synchronise.  Same results as ``k_steps`` calls
        of ``step_device``, bit for bit."""
        vp = C.c_void_p
        self._check(self._lib.hwy_rollout_device(self._h, int(k_steps), vp(d_actions), vp(d_obs), vp(d_reward),
                                                 vp(d_terminated), vp(d_truncated), vp(d_info_speed or None),
                                                 vp(d_info_crashed or None)))

    def rollout(self, actions):
        """hwy_rollout (host arrays): actions [K, E, A] -> (obs [K, E, A, ...], reward [K, E, A], terminated [K, E],
        truncated [K, E], info).  Raises KeyError for an action id outside the table, like ``step``."""
        acts = np.ascontiguousarray(np.asarray(actions, np.int32).reshape(-1, self.E, self.A))
        K, E, A = acts.shape[0], self.E, self.A
        obs = np.empty((K, E, A, *_abi.obs_shape(self.cfg)), np.float32)
        reward = np.empty((K, E, A), np.float64)
        term, trunc = np.empty((K, E), np.uint8), np.empty((K, E), np.uint8)
        speed, crashed = np.empty((K, E, A), np.float64), np.empty((K, E, A), np.uint8)
        self._check(self._lib.hwy_rollout(self._h, K, _ptr(acts), _ptr(obs), _ptr(reward), _ptr(term), _ptr(trunc),
                                          _ptr(speed), _ptr(crashed)))
        return obs, reward, term.astype(bool), trunc.astype(bool), {"speed": speed, "crashed": (crashed & 1).astype(bool),
                                                                    "arrived": (crashed & 2).astype(bool)}

    def step_frames(self, actions, n_frames: int):
        acts = None if actions is None else np.ascontiguousarray(np.asarray(actions, np.int32).reshape(self.E, self.A))
        self._check(self._lib.hwy_step_frames(self._h, _ptr(acts), int(n_frames)))

    def observe(self) -> np.ndarray:
        obs = np.empty((self.E, self.A, *_abi.obs_shape(self.cfg)), np.float32)
        self._check(self._lib.hwy_observe(self._h, _ptr(obs)))
        return obs

    # -- time-to-collision grid and finite-MDP planner (csrc/hwy_ttc.h) ---------------------------
    def _check_scope(self, rc: int):
        if rc == _abi.HWY_ERR_UNSUPPORTED:  # outside the entry point's scope: the project's NotImplementedError
            raise NotImplementedError(self._lib.hwy_last_error(self._h).decode())
        self._check(rc)

    _check_ttc = _check_scope  # (the name the planner entry points below were written with)

    def ttc_shape(self, params: _abi.HwyTtcParams) -> tuple:
        return (self.cfg.num_target_speeds, self.cfg.lanes_count, params.time_steps)

    def ttc_grid(self, params: _abi.HwyTtcParams) -> np.ndarray:
        """hwy_ttc_grid: compute_ttc_grid for every controlled vehicle, f32 [E, A, V, L, T] (values 0, 0.5, 1)."""
        grid = np.empty((self.E, self.A, *self.ttc_shape(params)), np.float32)
        self._check_ttc(self._lib.hwy_ttc_grid(self._h, C.byref(params), _ptr(grid)))
        return grid

    def mdp_plan(self, params: _abi.HwyTtcParams, return_q: bool = False, return_grid: bool = False):
        """hwy_mdp_plan: (actions int32 [E, A], Q f64 [E, A, 5] or None, grid f32 [E, A, V, L, T] or None)."""
        action = np.empty((self.E, self.A), np.int32)
        q = np.empty((self.E, self.A, 5), np.float64) if return_q else None
        grid = np.empty((self.E, self.A, *self.ttc_shape(params)), np.float32) if return_grid else None
        self._check_ttc(self._lib.hwy_mdp_plan(self._h, C.byref(params), _ptr(action), _ptr(q), _ptr(grid)))
        return action, q, grid

    def ttc_grid_device(self, params: _abi.HwyTtcParams, d_grid: int):
        """Enqueue hwy_ttc_grid_device on a raw device pointer; does not synchronise."""
        self._check_ttc(self._lib.hwy_ttc_grid_device(self._h, C.byref(params), C.c_void_p(d_grid)))

    def mdp_plan_device(self, params: _abi.HwyTtcParams, d_action: int, d_q: int = 0, d_grid: int = 0):
        """Enqueue hwy_mdp_plan_device on raw device pointers; does not synchronise."""
        vp = C.c_void_p
        self._check_ttc(self._lib.hwy_mdp_plan_device(self._h, C.byref(params), vp(d_action), vp(d_q or None), vp(d_grid or None)))

    # -- TimeToCollision observation (csrc/hwy_collision_obs.h) --------------------------------------
    def ttc_observe(self, params: _abi.HwyTtcParams) -> np.ndarray:
        """hwy_ttc_observe: TimeToCollisionObservation.observe for every controlled vehicle, f32 [E, A, 3, 3, T] (values 0, 0.5,
        1).  ``gamma`` and ``lane_change_reward`` of ``params`` are not read."""
        steps = params.time_steps if 1 <= params.time_steps <= _abi.HWY_MAX_TTC_STEPS else 1  # (the entry point refuses the rest)
        obs = np.empty((self.E, self.A, _abi.TTC_OBS_SIDE, _abi.TTC_OBS_SIDE, steps), np.float32)
        self._check_scope(self._lib.hwy_ttc_observe(self._h, C.byref(params), _ptr(obs)))
        return obs

    def ttc_observe_device(self, params: _abi.HwyTtcParams, d_obs: int):
        """Enqueue hwy_ttc_observe_device on a raw device pointer (float32 [E, A, 3, 3, T]); does not synchronise."""
        self._check_scope(self._lib.hwy_ttc_observe_device(self._h, C.byref(params), C.c_void_p(d_obs or None)))

    def step_same_step_ttc_device(self, params: _abi.HwyTtcParams, d_actions: int, d_obs: int, d_reward: int, d_terminated: int,
                                  d_truncated: int, d_info_speed: int = 0, d_info_crashed: int = 0, d_final_obs: int = 0,
                                  d_final_info_speed: int = 0, d_final_info_crashed: int = 0, d_final_mask: int = 0,
                                  d_action_mask: int = 0, d_final_action_mask: int = 0):
        """Enqueue hwy_step_same_step_ttc_device: ``step_same_step_device`` with the TimeToCollision window as ``d_obs`` and
        ``d_final_obs`` [E, A, 3, 3, T]; does not synchronise."""
        vp = C.c_void_p
        self._check_scope(self._lib.hwy_step_same_step_ttc_device(
            self._h, C.byref(params), vp(d_actions or None), vp(d_obs or None), vp(d_reward or None), vp(d_terminated or None),
            vp(d_truncated or None), vp(d_info_speed or None), vp(d_info_crashed or None), vp(d_final_obs or None),
            vp(d_final_info_speed or None), vp(d_final_info_crashed or None), vp(d_final_mask or None), vp(d_action_mask or None),
            vp(d_final_action_mask or None)))

    def rollout_ttc_device(self, params: _abi.HwyTtcParams, k_steps: int, d_actions: int, d_obs: int, d_reward: int, d_terminated: int,
                           d_truncated: int, d_info_speed: int = 0, d_info_crashed: int = 0):
        """Enqueue hwy_rollout_ttc_device: ``k_steps`` (step, observe) launch pairs on block k of every plane (d_obs
        [K, E, A, 3, 3, T]); does not synchronise.  ``k_steps`` 1: one step with the window as its observation; K steps give the
        results of K such calls, bit for bit."""
        vp = C.c_void_p
        self._check_scope(self._lib.hwy_rollout_ttc_device(self._h, C.byref(params), int(k_steps), vp(d_actions or None), vp(d_obs or None),
                                                           vp(d_reward or None), vp(d_terminated or None), vp(d_truncated or None),
                                                           vp(d_info_speed or None), vp(d_info_crashed or None)))

    # -- Lidar through a door of its own (csrc/hwy_lidar_door.h) --------------------------------------
    def lidar_observe(self, params: _abi.HwyLidarParams) -> np.ndarray:
        """hwy_lidar_observe: LidarObservation.observe of the current state for every controlled vehicle, f32 [E, A, cells, 2], on
        every scenario and next to whatever observation type the engine was created with."""
        cells = params.cells if 1 <= params.cells <= _abi.HWY_MAX_LIDAR_DOOR_CELLS else 1  # (the entry point refuses the rest)
        obs = np.empty((self.E, self.A, cells, 2), np.float32)
        self._check_scope(self._lib.hwy_lidar_observe(self._h, C.byref(params), _ptr(obs)))
        return obs

    def lidar_observe_device(self, params: _abi.HwyLidarParams, d_obs: int):
        """Enqueue hwy_lidar_observe_device on a raw device pointer (float32 [E, A, cells, 2]); does not synchronise."""
        self._check_scope(self._lib.hwy_lidar_observe_device(self._h, C.byref(params), C.c_void_p(d_obs or None)))

    def rollout_lidar_device(self, params: _abi.HwyLidarParams, k_steps: int, d_actions: int, d_obs: int, d_reward: int,
                             d_terminated: int, d_truncated: int, d_info_speed: int = 0, d_info_crashed: int = 0):
        """Enqueue hwy_rollout_lidar_device: ``k_steps`` (step, observe) launch pairs on block k of every plane (d_obs
        [K, E, A, cells, 2]); does not synchronise.  NotImplementedError on the intersection."""
        vp = C.c_void_p
        self._check_scope(self._lib.hwy_rollout_lidar_device(self._h, C.byref(params), int(k_steps), vp(d_actions or None), vp(d_obs or None),
                                                             vp(d_reward or None), vp(d_terminated or None), vp(d_truncated or None),
                                                             vp(d_info_speed or None), vp(d_info_crashed or None)))

    # -- environment fork and scoring of action sequences (csrc/hwy_lookahead.h) -------------------
    def fork_from(self, src: "Engine", branches: int = 1, source=None):
        """hwy_fork / hwy_fork_device: environment j of this engine becomes a copy of environment ``source[j]`` of ``src``
        (host indices, validated), or of ``j // branches``.  Without ``source`` the copy is only enqueued."""
        if source is None:
            self._check_ttc(self._lib.hwy_fork_device(self._h, src._h, int(branches), None))
            return
        idx = np.ascontiguousarray(source, dtype=np.int32)
        if idx.shape != (self.E,):
            raise ValueError(f"fork: source has shape {idx.shape}, this engine needs ({self.E},)")
        self._check_ttc(self._lib.hwy_fork(self._h, src._h, int(branches), _ptr(idx)))

    def fork_device(self, src: "Engine", branches: int = 1, d_src_env: int = 0):
        """Enqueue hwy_fork_device with a raw device pointer to the source indices (0: ``j // branches``); does not synchronise."""
        self._check_ttc(self._lib.hwy_fork_device(self._h, src._h, int(branches), C.c_void_p(d_src_env or None)))

    def score_device(self, k_steps: int, branches: int, gamma: float, d_first_action: int, d_reward: int, d_terminated: int,
                     d_truncated: int, d_return: int = 0, d_q: int = 0, d_best_action: int = 0, d_best_branch: int = 0):
        """Enqueue hwy_score_device on raw device pointers; does not synchronise."""
        vp = C.c_void_p
        self._check_ttc(self._lib.hwy_score_device(self._h, int(k_steps), int(branches), float(gamma), vp(d_first_action or None),
                                                   vp(d_reward or None), vp(d_terminated or None), vp(d_truncated or None),
                                                   vp(d_return or None), vp(d_q or None), vp(d_best_action or None),
                                                   vp(d_best_branch or None)))

    def score_rollout(self, actions, branches: int, gamma: float = 1.0) -> dict:
        """hwy_score_rollout (host arrays): actions [K, E*branches, A] are rolled out from the current state and folded.  Returns
        ``reward`` [K, E*branches, A], ``terminated`` / ``truncated`` [K, E*branches], ``returns`` [E, branches, A],
        ``best_branch`` [E, A] and, single agent, ``q`` [E, n_ids] and ``best_action`` [E].  Raises like ``rollout`` for an
        action id outside the table."""
        acts = np.ascontiguousarray(np.asarray(actions, np.int32).reshape(-1, self.E, self.A))
        K, EB, A, B = acts.shape[0], self.E, self.A, int(branches)
        if B < 1 or EB % B:
            raise ValueError(f"score_rollout: branches={B} does not divide the engine's {EB} environments")
        E, ids = EB // B, _abi.num_actions(self.cfg)
        out = {"reward": np.empty((K, EB, A), np.float64), "terminated": np.empty((K, EB), np.uint8),
               "truncated": np.empty((K, EB), np.uint8), "returns": np.empty((E, B, A), np.float64),
               "q": np.empty((E, ids), np.float64) if A == 1 else None, "best_action": np.empty(E, np.int32) if A == 1 else None,
               "best_branch": np.empty((E, A), np.int32)}
        self._check_ttc(self._lib.hwy_score_rollout(self._h, K, B, float(gamma), _ptr(acts), *(_ptr(out[k]) for k in (
            "reward", "terminated", "truncated", "returns", "q", "best_action", "best_branch"))))
        out["terminated"], out["truncated"] = out["terminated"].astype(bool), out["truncated"].astype(bool)
        return out

    # -- optimistic planning, one tree per environment (csrc/hwy_opd.h) -----------------------------
    def opd_plan(self, tree: "Engine", work: "Engine", params: _abi.HwyOpdParams) -> dict:
        """hwy_opd_plan (host arrays): ``action`` int32 [E], ``value`` / ``upper`` f64 [E], ``sequence`` int32 [E, X],
        ``expanded`` int32 [E].  ``tree`` / ``work``: engines of E * nodes and E * n_ids environments, auto-reset off."""
        E, X = self.E, params.budget // max(params.n_ids, 1)
        out = {"action": np.empty(E, np.int32), "value": np.empty(E, np.float64), "upper": np.empty(E, np.float64),
               "sequence": np.empty((E, X), np.int32), "expanded": np.empty(E, np.int32)}
        self._check_ttc(self._lib.hwy_opd_plan(self._h, tree._h, work._h, C.byref(params), *(_ptr(out[k]) for k in (
            "action", "value", "upper", "sequence", "expanded"))))
        return out

    def opd_plan_device(self, tree: "Engine", work: "Engine", params: _abi.HwyOpdParams, d_action: int, d_value: int = 0,
                        d_upper: int = 0, d_sequence: int = 0, d_expanded: int = 0):
        """Enqueue hwy_opd_plan_device on raw device pointers; does not synchronise."""
        vp = C.c_void_p
        self._check_ttc(self._lib.hwy_opd_plan_device(self._h, tree._h, work._h, C.byref(params), vp(d_action or None),
                                                      vp(d_value or None), vp(d_upper or None), vp(d_sequence or None),
                                                      vp(d_expanded or None)))

    # -- action mask (csrc/hwy_mask.h) ---------------------------------------------------------------
    def action_mask(self) -> np.ndarray:
        """hwy_action_mask: ``get_available_actions`` of every controlled vehicle, bool [E, A, n_ids] in the order of the engine's
        action table.  NotImplementedError on a DiscreteAction engine, like the reference's ``ActionType``."""
        mask = np.empty((self.E, self.A, _abi.num_actions(self.cfg)), np.uint8)
        self._check_scope(self._lib.hwy_action_mask(self._h, _ptr(mask)))
        return mask.astype(bool)

    def action_mask_device(self, d_mask: int):
        """Enqueue hwy_action_mask_device on a raw device pointer (uint8 [E, A, n_ids]); does not synchronise."""
        self._check_scope(self._lib.hwy_action_mask_device(self._h, C.c_void_p(d_mask or None)))

    # -- SameStep autoreset on the device (csrc/hwy_same_step.h) --------------------------------------
    def step_same_step_device(self, d_actions: int, d_obs: int, d_reward: int, d_terminated: int, d_truncated: int,
                              d_info_speed: int = 0, d_info_crashed: int = 0, d_final_obs: int = 0, d_final_info_speed: int = 0,
                              d_final_info_crashed: int = 0, d_final_mask: int = 0, d_action_mask: int = 0,
                              d_final_action_mask: int = 0):
        """Enqueue hwy_step_same_step_device on raw device pointers: one policy step, the terminal rows of the environments that
        ended stashed into the ``final`` planes (read them under ``d_final_mask``), their next episode started in the same call;
        does not synchronise.  Needs ``set_autoreset(True, ...)``.  NotImplementedError on the intersection scenario, and for a
        mask pointer on a DiscreteAction engine."""
        vp = C.c_void_p
        self._check_scope(self._lib.hwy_step_same_step_device(
            self._h, vp(d_actions or None), vp(d_obs or None), vp(d_reward or None), vp(d_terminated or None), vp(d_truncated or None),
            vp(d_info_speed or None), vp(d_info_crashed or None), vp(d_final_obs or None), vp(d_final_info_speed or None),
            vp(d_final_info_crashed or None), vp(d_final_mask or None), vp(d_action_mask or None), vp(d_final_action_mask or None)))

    # -- continuous throttle and steering of a direct-control engine (csrc/hwy_act.h) -------------------
    def _check_continuous(self, rc: int):
        if rc == _abi.HWY_ERR_ACTION:  # a NaN or an infinity: no member of Box(-1, 1, (size,), float32)
            raise ValueError(self._lib.hwy_last_error(self._h).decode())
        self._check_scope(rc)

    def _continuous_actions(self, params: _abi.HwyContinuousParams, actions, lead=()) -> np.ndarray:
        """``actions`` as the contiguous float32 [*lead, E, A, size] the entry points read.  A float64 array is ROUNDED to float32
        here: the reference's ``Box(-1, 1, (size,), float32)`` does not contain it either, and its mapping is defined on float32."""
        return np.ascontiguousarray(np.asarray(actions, np.float32).reshape(*lead, self.E, self.A, params.size))

    def act_continuous(self, params: _abi.HwyContinuousParams, actions):
        """hwy_act_continuous: the act kernel alone.  ``actions`` [E, A, size] are clipped to [-1, 1], mapped onto the ranges of
        ``params`` as the reference's ``ContinuousAction.get_action`` maps a float32 action, and stored as the (acceleration,
        steering) pairs ``get_controls`` reads.  ValueError for a non-finite component."""
        a = self._continuous_actions(params, actions)
        self._check_continuous(self._lib.hwy_act_continuous(self._h, C.byref(params), _ptr(a)))

    def act_continuous_device(self, params: _abi.HwyContinuousParams, d_actions: int):
        """Enqueue hwy_act_continuous_device on a raw device pointer (float32 [E, A, size]); does not synchronise.  A row with a
        non-finite component leaves its stored pair as it is."""
        self._check_continuous(self._lib.hwy_act_continuous_device(self._h, C.byref(params), C.c_void_p(d_actions or None)))

    def step_continuous(self, params: _abi.HwyContinuousParams, actions):
        """hwy_step_continuous (host arrays): ``step`` with float actions [E, A, size] in place of ids -- the act kernel, then the
        engine's own step launch on the pair it stored.  A float64 array is rounded to float32 first.  ValueError for a
        non-finite component, before anything runs."""
        E, A = self.E, self.A
        a = self._continuous_actions(params, actions)
        obs = np.empty((E, A, *_abi.obs_shape(self.cfg)), np.float32)
        reward = np.empty((E, A), np.float64)
        term, trunc = np.empty(E, np.uint8), np.empty(E, np.uint8)
        speed, crashed = np.empty((E, A), np.float64), np.empty((E, A), np.uint8)
        self._check_continuous(self._lib.hwy_step_continuous(self._h, C.byref(params), _ptr(a), _ptr(obs), _ptr(reward), _ptr(term),
                                                             _ptr(trunc), _ptr(speed), _ptr(crashed)))
        return obs, reward, term.astype(bool), trunc.astype(bool), {"speed": speed, "crashed": (crashed & 1).astype(bool),
                                                                    "arrived": (crashed & 2).astype(bool)}

    def rollout_continuous(self, params: _abi.HwyContinuousParams, actions):
        """hwy_rollout_continuous (host arrays): actions [K, E, A, size] -> the tuple of ``rollout``.  K (act, step) launch pairs
        enqueued by one call; the results of K ``step_continuous`` calls, bit for bit."""
        a = self._continuous_actions(params, actions, lead=(-1,))
        K, E, A = a.shape[0], self.E, self.A
        obs = np.empty((K, E, A, *_abi.obs_shape(self.cfg)), np.float32)
        reward = np.empty((K, E, A), np.float64)
        term, trunc = np.empty((K, E), np.uint8), np.empty((K, E), np.uint8)
        speed, crashed = np.empty((K, E, A), np.float64), np.empty((K, E, A), np.uint8)
        self._check_continuous(self._lib.hwy_rollout_continuous(self._h, C.byref(params), K, _ptr(a), _ptr(obs), _ptr(reward),
                                                                _ptr(term), _ptr(trunc), _ptr(speed), _ptr(crashed)))
        return obs, reward, term.astype(bool), trunc.astype(bool), {"speed": speed, "crashed": (crashed & 1).astype(bool),
                                                                    "arrived": (crashed & 2).astype(bool)}

    def step_continuous_device(self, params: _abi.HwyContinuousParams, d_actions: int, d_obs: int, d_reward: int, d_terminated: int,
                               d_truncated: int, d_info_speed: int = 0, d_info_crashed: int = 0):
        """Enqueue hwy_step_continuous_device on raw device pointers (``d_actions``: float32 [E, A, size]); does not synchronise."""
        vp = C.c_void_p
        self._check_continuous(self._lib.hwy_step_continuous_device(
            self._h, C.byref(params), vp(d_actions or None), vp(d_obs or None), vp(d_reward or None), vp(d_terminated or None),
            vp(d_truncated or None), vp(d_info_speed or None), vp(d_info_crashed or None)))

    def rollout_continuous_device(self, params: _abi.HwyContinuousParams, k_steps: int, d_actions: int, d_obs: int, d_reward: int,
                                  d_terminated: int, d_truncated: int, d_info_speed: int = 0, d_info_crashed: int = 0):
        """Enqueue hwy_rollout_continuous_device (``d_actions``: float32 [K, E, A, size], block k of every plane belongs to step k):
        ``k_steps`` (act, step) launch pairs, no host round trip; does not synchronise."""
        vp = C.c_void_p
        self._check_continuous(self._lib.hwy_rollout_continuous_device(
            self._h, C.byref(params), int(k_steps), vp(d_actions or None), vp(d_obs or None), vp(d_reward or None),
            vp(d_terminated or None), vp(d_truncated or None), vp(d_info_speed or None), vp(d_info_crashed or None)))

    def step_same_step_continuous_device(self, params: _abi.HwyContinuousParams, d_actions: int, d_obs: int, d_reward: int,
                                         d_terminated: int, d_truncated: int, d_info_speed: int = 0, d_info_crashed: int = 0,
                                         d_final_obs: int = 0, d_final_info_speed: int = 0, d_final_info_crashed: int = 0,
                                         d_final_mask: int = 0, d_action_mask: int = 0, d_final_action_mask: int = 0):
        """Enqueue hwy_step_same_step_continuous_device: ``step_same_step_device`` with float actions [E, A, size] in place of ids."""
        vp = C.c_void_p
        self._check_continuous(self._lib.hwy_step_same_step_continuous_device(
            self._h, C.byref(params), vp(d_actions or None), vp(d_obs or None), vp(d_reward or None), vp(d_terminated or None),
            vp(d_truncated or None), vp(d_info_speed or None), vp(d_info_crashed or None), vp(d_final_obs or None),
            vp(d_final_info_speed or None), vp(d_final_info_crashed or None), vp(d_final_mask or None), vp(d_action_mask or None),
            vp(d_final_action_mask or None)))

    # -- the float door into fork / rollout / score, and the CEM planner on it (csrc/hwy_cem.h) ----------
    def score_rollout_continuous(self, params: _abi.HwyContinuousParams, actions, branches: int, gamma: float = 1.0) -> dict:
        """hwy_score_rollout_continuous (host arrays): float actions [K, E*branches, A, size] are rolled out from the current state
        (K act + step launch pairs) and folded.  Returns ``reward`` [K, E*branches, A], ``terminated`` / ``truncated``
        [K, E*branches], ``returns`` [E, branches, A] and ``best_branch`` [E, A].  ValueError for a non-finite component."""
        a = self._continuous_actions(params, actions, lead=(-1,))
        K, EB, A, B = a.shape[0], self.E, self.A, int(branches)
        if B < 1 or EB % B:
            raise ValueError(f"score_rollout_continuous: branches={B} does not divide the engine's {EB} environments")
        E = EB // B
        out = {"reward": np.empty((K, EB, A), np.float64), "terminated": np.empty((K, EB), np.uint8),
               "truncated": np.empty((K, EB), np.uint8), "returns": np.empty((E, B, A), np.float64),
               "best_branch": np.empty((E, A), np.int32)}
        self._check_continuous(self._lib.hwy_score_rollout_continuous(self._h, C.byref(params), K, B, float(gamma), _ptr(a), *(
            _ptr(out[k]) for k in ("reward", "terminated", "truncated", "returns", "best_branch"))))
        out["terminated"], out["truncated"] = out["terminated"].astype(bool), out["truncated"].astype(bool)
        return out

    def cem_plan(self, work: "Engine", params: _abi.HwyContinuousParams, cem: _abi.HwyCemParams, init_mean=None, debug: bool = False) -> dict:
        """hwy_cem_plan (host arrays): ``action`` f32 [E, size], ``best_return`` f64 [E], ``mean`` / ``std`` f64 [E, K, size],
        ``best_sequence`` f32 [E, K, size] and, with ``debug``, ``noise`` f64 / ``samples`` f32 [I, E, B, K, size] and ``elites`` int32 [I, E, M].  ``work``: an
        engine of E * population environments, auto-reset off.  ``init_mean``: f64 [E, K, size] or None (zeros); ValueError for a
        non-finite entry."""
        E, B, K, I, size = self.E, cem.population, cem.horizon, cem.iterations, params.size
        im = None
        if init_mean is not None:
            im = np.ascontiguousarray(init_mean, dtype=np.float64)
            if im.shape != (E, K, size):
                raise ValueError(f"cem_plan: init_mean has shape {im.shape}, this search needs {(E, K, size)}")
        out = {"action": np.empty((E, size), np.float32), "best_return": np.empty(E, np.float64), "mean": np.empty((E, K, size), np.float64),
               "std": np.empty((E, K, size), np.float64), "best_sequence": np.empty((E, K, size), np.float32),
               "noise": np.empty((I, E, B, K, size), np.float64) if debug else None,
               "samples": np.empty((I, E, B, K, size), np.float32) if debug else None,
               "elites": np.empty((I, E, cem.elites), np.int32) if debug else None}
        self._check_continuous(self._lib.hwy_cem_plan(self._h, work._h, C.byref(params), C.byref(cem), _ptr(im), *(
            _ptr(out[k]) for k in ("action", "best_return", "mean", "std", "best_sequence", "noise", "samples", "elites"))))
        return out

    def cem_plan_device(self, work: "Engine", params: _abi.HwyContinuousParams, cem: _abi.HwyCemParams, d_action: int,
                        d_init_mean: int = 0, d_best_return: int = 0, d_mean: int = 0, d_std: int = 0, d_best_sequence: int = 0,
                        d_noise: int = 0, d_samples: int = 0, d_elites: int = 0):
        """Enqueue hwy_cem_plan_device on raw device pointers; does not synchronise."""
        vp = C.c_void_p
        self._check_continuous(self._lib.hwy_cem_plan_device(
            self._h, work._h, C.byref(params), C.byref(cem), vp(d_init_mean or None), vp(d_action or None), vp(d_best_return or None),
            vp(d_mean or None), vp(d_std or None), vp(d_best_sequence or None), vp(d_noise or None), vp(d_samples or None),
            vp(d_elites or None)))

    # -- reset --------------------------------------------------------------------------------
    def reset(self, seeds=None, mask=None, ego_spacing=2.0, vehicles_density=1.0, initial_lane_id=-1, base_seed=0):
        """Device-side spawn (counter-based RNG; NOT numpy's stream -- see spawn.py for that)."""
        if seeds is None:
            seeds = np.uint64(base_seed) + np.arange(self.E, dtype=np.uint64)
        sd = np.ascontiguousarray(seeds, np.uint64)
        mk = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        obs = np.zeros((self.E, self.A, *_abi.obs_shape(self.cfg)), np.float32)
        self._check(self._lib.hwy_reset(self._h, _ptr(mk), _ptr(sd), float(ego_spacing), float(vehicles_density),
                                        int(initial_lane_id), _ptr(obs)))
        return obs

    def set_autoreset(self, enabled: bool, base_seed: int = 0, ego_spacing=2.0, vehicles_density=1.0,
                      initial_lane_id=-1):
        self._check(self._lib.hwy_set_autoreset(self._h, int(bool(enabled)), C.c_uint64(base_seed), float(ego_spacing),
                                                float(vehicles_density), int(initial_lane_id)))

    def debug_math(self, op: int, x) -> np.ndarray:
        """Evaluate one of the kernel's math routines (csrc/hwy_math.h) on the device (self-test hook)."""
        xin = np.ascontiguousarray(x, np.float64).ravel()
        out = np.empty_like(xin)
        self._check(self._lib.hwy_debug_math(self._h, int(op), _ptr(xin), _ptr(out), xin.size))
        return out.reshape(np.shape(x))

    # -- misc ---------------------------------------------------------------------------------
    COUNTERS = ("ix_spawns", "ix_spawns_dropped", "nonfinite_stores")

    def counters(self, reset: bool = False) -> dict:
        """Event counters (hwy_get_counters): intersection scenario, device traffic -- spawns performed, and spawns
        DROPPED because all ``max_vehicles`` slots were taken (the reference's vehicle list is unbounded)."""
        out = (C.c_uint64 * 8)()
        self._check(self._lib.hwy_get_counters(self._h, out, 8, int(bool(reset))))
        return {k: int(out[i]) for i, k in enumerate(self.COUNTERS)}

    def set_block_order(self, env_of_block=None):
        """hwy_set_block_order: workgroup b of the following step launches steps environment ``env_of_block[b]`` (a permutation;
        None = identity).  A placement of the environments on the SIMDs -- never changes a result."""
        if env_of_block is None:
            self._check(self._lib.hwy_set_block_order(self._h, None))
            return
        a = np.ascontiguousarray(env_of_block, np.int32)
        if a.shape != (self.E,):
            raise ValueError(f"env_of_block must have shape ({self.E},)")
        self._check(self._lib.hwy_set_block_order(self._h, _ptr(a)))

    # -- multi-GPU: RCCL gather behind the ABI (one process per GPU) -----------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        """Rank 0: the 128-byte RCCL id every rank passes to ``comm_init`` (ship it by any means)."""
        lib = _lib.load()
        buf = (C.c_uint8 * 128)()
        rc = lib.hwy_comm_unique_id(buf)
        if rc != 0:
            raise EngineError(f"hwy_comm_unique_id: {lib.hwy_last_error(None).decode()}")
        return bytes(buf)

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._check(self._lib.hwy_comm_init(self._h, buf, int(rank), int(world)))

    def gather(self, d_send: int, d_recv: int, nbytes: int, root: int = 0):
        """Enqueue ncclGather of ``nbytes`` bytes per rank (device pointers) on the engine's stream."""
        self._check(self._lib.hwy_gather(self._h, C.c_void_p(d_send), C.c_void_p(d_recv or None), C.c_size_t(nbytes), int(root)))

    def comm_destroy(self):
        self._check(self._lib.hwy_comm_destroy(self._h))

    def sync(self):
        self._check(self._lib.hwy_sync(self._h))

    def profile_enable(self, every: int = 1):
        """HIP-event timing of every `every`-th step-kernel launch (0 / False = off)."""
        self._check(self._lib.hwy_profile_enable(self._h, int(every)))

    def profile_read(self):
        ms, n = C.c_double(), C.c_int64()
        self._check(self._lib.hwy_profile_read(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def prio_turn(self):
        """(turn, state) of hwy_get_prio_turn: the issue-priority turn in use (tune_prio_shift's encoding) and whether the engine
        chose it itself (0 = no selection, 1 = still sampling its first launches, 2 = chosen)."""
        turn, state = C.c_int32(), C.c_int32()
        self._check(self._lib.hwy_get_prio_turn(self._h, C.byref(turn), C.byref(state)))
        return turn.value, state.value


def step_shapes(on: bool | None = None) -> bool:
    """hwy_step_shapes: whether step launches may run the kernel builds compiled for the registered configurations (process-wide;
    ``None`` only asks).  Returns the setting that was in force."""
    return bool(_lib.load().hwy_step_shapes(-1 if on is None else int(bool(on))))


def last_step_shape() -> int:
    """hwy_last_step_shape: 0 = the last step launch ran the generic kernel, 1 / 2 = highway-fast-v0 on 3 / 4 lanes, 3 = highway-v0."""
    return int(_lib.load().hwy_last_step_shape())


def device_count() -> int:
    return _lib.load().hwy_device_count()
