"""The parking scenario (the reference's ``ParkingEnv``, envs/parking_env.py) on the MI355X: goal-conditioned continuous control.

E environments of one ``ContinuousAction`` ego, up to 26 parked vehicles and four walls, advanced by a kernel of its own
(``csrc/hwy_park.h``, one thread per environment) behind the C-ABI of ``include/hwy_park.h`` -- a door next to the step engine.

* ``BatchedParkingEnv(config, num_envs)``: ``reset`` / ``step(actions)`` / ``rollout(actions[K])`` / ``compute_reward`` /
  ``get_state`` / ``set_state`` / ``plan_cem`` / ``score_sequences`` (sampling MPC, ``csrc/hwy_park_cem.h``: the whole search of
  every environment in one launch, a wavefront per environment and a candidate per lane) / ``plan_mppi`` (the MPPI planner of
  ``csrc/hwy_park_mppi.h``, built the same way); observations are the reference's dict of ``observation`` / ``achieved_goal`` / ``desired_goal``,
  float32 ``[E, 6]`` each.
* ``ParkingEnv``, ``ParkingEnvActionRepeat``, ``ParkingEnvParkedVehicles``: single-environment drop-ins with ``info["is_success"]``.
* ``REGISTRY`` / ``register_envs``: the ids ``parking-v0``, ``parking-ActionRepeat-v0`` and ``parking-parked-v0``.  They live here
  and not in ``envs.REGISTRY``, which lists the ids of the step engine; ``HighwayVectorEnv("parking-v0", E)`` resolves them.
* ``ParkingVectorEnv``: the vector front end (NextStep autoreset; ``output="torch"``: device tensors in and out).

Outside the scope (several agents, ``dynamical``, ``speed_range``, ``clip: False``, one axis only, other features or observation
types, ``p != 0.5``, rendering) everything raises ``NotImplementedError`` before the device is touched.  There is no CPU fallback.
"""
from __future__ import annotations

import copy
import ctypes as C

import numpy as np

try:  # optional
    import gymnasium as _gym
    _GYM_BASES = (_gym.Env,)
    _VecBase = _gym.vector.VectorEnv
except Exception:  # pragma: no cover - gymnasium is absent in the build image
    _gym = None
    _GYM_BASES = ()
    _VecBase = object

SPOTS, MAX_PARKED = 28, 26
EGO_FIELDS = ("x", "y", "heading", "speed", "acceleration", "steering", "impact_x", "impact_y", "time")
INT_FIELDS = ("flags", "steps", "episode", "goal", "occupied", "struck", "parked_crashed", "parked_impact")
PARKED_FIELDS = ("parked_x", "parked_y", "parked_impact_x", "parked_impact_y")
F_CRASHED, F_HAS_IMPACT, F_DONE = 1, 2, 4
S_TERMINATED, S_TRUNCATED, S_SUCCESS, S_CRASHED = 1, 2, 4, 8
FEATURES = ["x", "y", "vx", "vy", "cos_h", "sin_h"]
EXPORTS = ["hwy_park_create", "hwy_park_destroy", "hwy_park_last_error", "hwy_park_reset", "hwy_park_set_autoreset",
           "hwy_park_set_state", "hwy_park_get_state", "hwy_park_advance", "hwy_park_advance_device", "hwy_park_observe",
           "hwy_park_goal_reward_device", "hwy_park_goal_reward", "hwy_park_sync", "hwy_park_cem_plan_device", "hwy_park_cem_plan",
           "hwy_park_score_device", "hwy_park_score", "hwy_park_mppi_plan_device", "hwy_park_mppi_plan"]
CEM_MAX_POP, CEM_MAX_HORIZON, CEM_MAX_SAMPLES, CEM_MAX_ITERATIONS = 256, 32, 4096, 16  # include/hwy_park.h: HWY_PARK_CEM_*
PLAN_BYTES_PER_ENV = 8 * 4 * MAX_PARKED * 64  # the candidates' struck bodies, f64 [4][26][64] per environment


class HwyParkConfig(C.Structure):
    """ctypes mirror of ``hwy_park_config`` (include/hwy_park.h)."""
    _fields_ = [("struct_size", C.c_int32), ("num_envs", C.c_int32), ("vehicles_count", C.c_int32), ("add_walls", C.c_int32),
                ("frames", C.c_int32), ("autoreset", C.c_int32), ("dt", C.c_double), ("policy_dt", C.c_double),
                ("duration", C.c_double), ("reward_weights", C.c_double * 6), ("scales", C.c_double * 6),
                ("success_goal_reward", C.c_double), ("collision_reward", C.c_double), ("acceleration_range", C.c_double * 2),
                ("steering_range", C.c_double * 2), ("base_seed", C.c_uint64)]


def parking_default_config() -> dict:
    """``ParkingEnv.default_config()`` (parking_env.py:88-116) without the rendering keys."""
    return {"observation": {"type": "KinematicsGoal", "features": list(FEATURES), "scales": [100, 100, 5, 5, 1, 1], "normalize": False},
            "action": {"type": "ContinuousAction"}, "reward_weights": [1, 0.3, 0, 0, 0.02, 0.02], "success_goal_reward": 0.12,
            "collision_reward": -5, "steering_range": float(np.deg2rad(45)), "simulation_frequency": 15, "policy_frequency": 5,
            "duration": 100, "controlled_vehicles": 1, "vehicles_count": 0, "add_walls": True}


def make_park_config(config: dict, num_envs: int, autoreset: bool = False, base_seed: int = 0) -> HwyParkConfig:
    """The kernel's configuration of a ParkingEnv config dict; ``NotImplementedError`` outside the scope of the module docstring."""
    def out(msg):
        raise NotImplementedError(f"parking: {msg} is outside the scope of the device kernel")
    if config.get("controlled_vehicles", 1) != 1:
        out("controlled_vehicles != 1 (several agents)")
    if config.get("render_mode") or config.get("offscreen_rendering"):
        out("rendering")
    obs = config["observation"]
    if obs.get("type") != "KinematicsGoal":
        out(f"observation type {obs.get('type')!r}")
    if list(obs.get("features", FEATURES)) != FEATURES or set(obs) - {"type", "features", "scales", "normalize"}:
        out("a KinematicsGoal observation with other features or options")
    act = config["action"]
    if act.get("type") != "ContinuousAction":
        out(f"action type {act.get('type')!r}")
    if act.get("dynamical", False) or act.get("speed_range") or not act.get("clip", True):
        out("dynamical / speed_range / clip: False")
    if not act.get("longitudinal", True) or not act.get("lateral", True):
        out("a ContinuousAction with one axis only")
    if set(act) - {"type", "acceleration_range", "steering_range", "speed_range", "longitudinal", "lateral", "dynamical", "clip"}:
        out("unknown ContinuousAction options")
    # (the config's top-level "steering_range" is never read by ContinuousAction: the action's own range steers)
    a_rng = act.get("acceleration_range") or (-5, 5.0)
    s_rng = act.get("steering_range") or (-np.pi / 4, np.pi / 4)
    if max(abs(float(s_rng[0])), abs(float(s_rng[1]))) > np.pi / 3:
        out("a steering_range beyond +-pi/3")
    vc = config["vehicles_count"]
    if not (isinstance(vc, (int, np.integer)) and 0 <= vc <= MAX_PARKED):
        out("vehicles_count outside 0 .. 26")
    sf, pf = config["simulation_frequency"], config["policy_frequency"]
    frames = int(sf // pf)
    if sf <= 0 or pf <= 0 or frames * pf != sf or not 1 <= frames <= 15:
        out("a simulation_frequency / policy_frequency ratio that is not an integer in 1 .. 15")
    if len(config["reward_weights"]) != 6 or len(obs.get("scales", [])) != 6:
        out("reward_weights / scales that are not six values")
    c = HwyParkConfig()
    c.struct_size, c.num_envs, c.vehicles_count, c.add_walls = C.sizeof(HwyParkConfig), int(num_envs), int(vc), int(bool(config["add_walls"]))
    c.frames, c.autoreset, c.dt, c.policy_dt, c.duration = frames, int(bool(autoreset)), 1 / sf, 1 / pf, float(config["duration"])
    c.reward_weights[:], c.scales[:] = [float(x) for x in config["reward_weights"]], [float(x) for x in obs["scales"]]
    c.success_goal_reward, c.collision_reward = float(config["success_goal_reward"]), float(config["collision_reward"])
    c.acceleration_range[:], c.steering_range[:] = [float(x) for x in a_rng], [float(x) for x in s_rng]
    c.base_seed = int(base_seed) & (2 ** 64 - 1)
    return c


def park_cem_params(population, elites, iterations, horizon, gamma, init_std, min_std, alpha, seed):
    """``hwy_cem_params`` of a search on parking: ``_abi.cem_params`` under parking's own caps.  ValueError for what
    ``hwy_park_cem_plan`` rejects as HWY_PARK_ERR_INVALID_ARG."""
    from . import _abi
    cem = _abi.cem_params(population, elites, iterations, horizon, gamma, init_std, min_std, alpha, seed)
    if cem.population > CEM_MAX_POP:
        raise ValueError(f"parking: population ({cem.population}) must be at most {CEM_MAX_POP}")
    if cem.horizon > CEM_MAX_HORIZON:
        raise ValueError(f"parking: horizon ({cem.horizon}) must be at most {CEM_MAX_HORIZON}")
    if cem.population * cem.horizon > CEM_MAX_SAMPLES:
        raise ValueError(f"parking: population * horizon ({cem.population * cem.horizon}) must be at most {CEM_MAX_SAMPLES}")
    if cem.iterations > CEM_MAX_ITERATIONS:
        raise ValueError(f"parking: iterations ({cem.iterations}) must be at most {CEM_MAX_ITERATIONS}")
    return cem


class HwyParkMppiParams(C.Structure):
    """ctypes mirror of ``hwy_park_mppi_params`` (include/hwy_park.h)."""
    _fields_ = [("struct_size", C.c_int32), ("population", C.c_int32), ("iterations", C.c_int32), ("horizon", C.c_int32),
                ("gamma", C.c_double), ("noise_std", C.c_double), ("temperature", C.c_double), ("beta", C.c_double),
                ("beta_c", C.c_double), ("alpha", C.c_double), ("seed", C.c_uint64)]


def park_mppi_params(population, iterations, horizon, gamma, noise_std, temperature, beta, alpha, seed) -> HwyParkMppiParams:
    """``hwy_park_mppi_params`` of an MPPI search on parking, ``beta_c = sqrt(1 - beta * beta)`` in float64 included.  ValueError for
    what ``hwy_park_mppi_plan`` rejects as HWY_PARK_ERR_INVALID_ARG."""
    B, I, K = int(population), int(iterations), int(horizon)
    if not 1 <= B <= CEM_MAX_POP:
        raise ValueError(f"parking: population ({B}) must be in [1, {CEM_MAX_POP}]")
    if not 1 <= K <= CEM_MAX_HORIZON:
        raise ValueError(f"parking: horizon ({K}) must be in [1, {CEM_MAX_HORIZON}]")
    if B * K > CEM_MAX_SAMPLES:
        raise ValueError(f"parking: population * horizon ({B * K}) must be at most {CEM_MAX_SAMPLES}")
    if not 1 <= I <= CEM_MAX_ITERATIONS:
        raise ValueError(f"parking: iterations ({I}) must be in [1, {CEM_MAX_ITERATIONS}]")
    if not np.isfinite(gamma):
        raise ValueError("gamma must be finite")
    if not (np.isfinite(noise_std) and noise_std >= 0):
        raise ValueError("noise_std must be finite and >= 0")
    if not (np.isfinite(temperature) and temperature > 0):
        raise ValueError("temperature must be finite and > 0")
    if not 0.0 <= beta < 1.0:
        raise ValueError("beta must be in [0, 1)")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError("alpha must be in [0, 1]")
    p = HwyParkMppiParams()
    p.struct_size, p.population, p.iterations, p.horizon = C.sizeof(HwyParkMppiParams), B, I, K
    p.gamma, p.noise_std, p.temperature, p.alpha = float(gamma), float(noise_std), float(temperature), float(alpha)
    p.beta, p.beta_c = float(beta), float(np.sqrt(np.float64(1.0) - np.float64(beta) * np.float64(beta)))
    p.seed = int(seed) & (2 ** 64 - 1)
    return p


_park_lib = None


def load():
    """The parking entry points of libhwy_engine.so (raises when the library is missing: no CPU fallback)."""
    global _park_lib
    if _park_lib is None:
        from . import _lib
        lib = _lib.load()
        vp, i32 = C.c_void_p, C.c_int32
        lib.hwy_park_create.argtypes = [C.POINTER(HwyParkConfig), C.c_int, vp, C.POINTER(vp)]
        lib.hwy_park_destroy.argtypes = [vp]
        lib.hwy_park_last_error.argtypes, lib.hwy_park_last_error.restype = [vp], C.c_char_p
        lib.hwy_park_reset.argtypes = [vp, vp, vp, vp]
        lib.hwy_park_set_autoreset.argtypes = [vp, i32, C.c_uint64]
        lib.hwy_park_set_state.argtypes = lib.hwy_park_get_state.argtypes = [vp, vp, vp, vp, vp]
        lib.hwy_park_advance.argtypes = lib.hwy_park_advance_device.argtypes = [vp, i32] + [vp] * 6
        lib.hwy_park_observe.argtypes = [vp, vp]
        lib.hwy_park_goal_reward.argtypes = lib.hwy_park_goal_reward_device.argtypes = [vp, C.c_int64, vp, vp, vp]
        lib.hwy_park_sync.argtypes = [vp]
        lib.hwy_park_cem_plan.argtypes = lib.hwy_park_cem_plan_device.argtypes = [vp] * 12
        lib.hwy_park_mppi_plan.argtypes = lib.hwy_park_mppi_plan_device.argtypes = [vp] * 12
        lib.hwy_park_score.argtypes = lib.hwy_park_score_device.argtypes = [vp, i32, i32, C.c_double] + [vp] * 4
        _park_lib = lib
    return _park_lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class ParkEngine:
    """One ``hwy_park`` handle: the planes of E environments and a HIP stream."""

    def __init__(self, cfg: HwyParkConfig, device: int = 0, stream: int | None = None):
        self.lib, self.cfg, self.E = load(), cfg, cfg.num_envs
        h = C.c_void_p()
        rc = self.lib.hwy_park_create(C.byref(cfg), device, stream, C.byref(h))
        if rc:
            raise RuntimeError(f"hwy_park_create: {self.lib.hwy_park_last_error(None).decode()}")
        self.h = h

    def _check(self, rc):
        if rc:
            raise RuntimeError(self.lib.hwy_park_last_error(self.h).decode())

    def close(self):
        if self.h:
            self.lib.hwy_park_destroy(self.h)
            self.h = None

    def set_autoreset(self, enabled: bool, base_seed: int):
        self._check(self.lib.hwy_park_set_autoreset(self.h, int(bool(enabled)), int(base_seed) & (2 ** 64 - 1)))

    def reset(self, seeds=None, mask=None):
        obs = np.empty((self.E, 3, 6), np.float32)
        seeds = None if seeds is None else np.ascontiguousarray(seeds, np.uint64)
        mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self._check(self.lib.hwy_park_reset(self.h, _ptr(mask), _ptr(seeds), _ptr(obs)))
        return obs

    def observe(self):
        obs = np.empty((self.E, 3, 6), np.float32)
        self._check(self.lib.hwy_park_observe(self.h, _ptr(obs)))
        return obs

    def set_state(self, st: dict):
        E = self.E
        ego = np.ascontiguousarray(np.stack([np.asarray(st[k], np.float64).reshape(E) for k in EGO_FIELDS]))
        ints = np.ascontiguousarray(np.stack([np.asarray(st[k]).astype(np.int64).astype(np.int32).reshape(E) for k in INT_FIELDS]))
        order = np.ascontiguousarray(np.asarray(st["order"], np.uint8).reshape(E, MAX_PARKED).T)
        parked = np.ascontiguousarray(np.stack([np.asarray(st[k], np.float64).reshape(E, MAX_PARKED).T for k in PARKED_FIELDS]))
        self._check(self.lib.hwy_park_set_state(self.h, _ptr(ego), _ptr(ints), _ptr(order), _ptr(parked)))

    def get_state(self) -> dict:
        E = self.E
        ego, ints = np.empty((len(EGO_FIELDS), E)), np.empty((len(INT_FIELDS), E), np.int32)
        order, parked = np.empty((MAX_PARKED, E), np.uint8), np.empty((len(PARKED_FIELDS), MAX_PARKED, E))
        self._check(self.lib.hwy_park_get_state(self.h, _ptr(ego), _ptr(ints), _ptr(order), _ptr(parked)))
        st = {k: ego[i].copy() for i, k in enumerate(EGO_FIELDS)}
        st.update({k: ints[i].copy() for i, k in enumerate(INT_FIELDS)})
        st["order"] = order.T.copy()
        st.update({k: parked[i].T.copy() for i, k in enumerate(PARKED_FIELDS)})
        return st

    def advance(self, actions, per_step: bool = False):
        """``actions`` float32 [K, E, 2] -> (obs [E, 3, 6], reward [E], flags [E]) of the last step, and with ``per_step`` the reward
        [K, E] and flags [K, E] of every step."""
        a = np.ascontiguousarray(actions, np.float32)
        K = a.shape[0]
        if a.shape != (K, self.E, 2):
            raise ValueError(f"actions must be [K, {self.E}, 2]")
        obs, reward, flags = np.empty((self.E, 3, 6), np.float32), np.empty(self.E), np.empty(self.E, np.uint8)
        sr, sf = (np.empty((K, self.E)), np.empty((K, self.E), np.uint8)) if per_step else (None, None)
        self._check(self.lib.hwy_park_advance(self.h, K, _ptr(a), _ptr(obs), _ptr(reward), _ptr(flags), _ptr(sr), _ptr(sf)))
        return (obs, reward, flags, sr, sf) if per_step else (obs, reward, flags)

    def advance_device(self, k_steps, d_actions, d_obs, d_reward, d_flags, d_step_reward=None, d_step_flags=None):
        self._check(self.lib.hwy_park_advance_device(self.h, int(k_steps), d_actions, d_obs, d_reward, d_flags, d_step_reward, d_step_flags))

    def goal_reward(self, achieved, desired):
        a, d = np.ascontiguousarray(achieved, np.float64).reshape(-1, 6), np.ascontiguousarray(desired, np.float64).reshape(-1, 6)
        out = np.empty(len(a))
        self._check(self.lib.hwy_park_goal_reward(self.h, len(a), _ptr(a), _ptr(d), _ptr(out)))
        return out

    def goal_reward_device(self, m, d_achieved, d_desired, d_out):
        self._check(self.lib.hwy_park_goal_reward_device(self.h, int(m), d_achieved, d_desired, d_out))

    def sync(self):
        self._check(self.lib.hwy_park_sync(self.h))

    def score(self, actions, gamma: float = 1.0, per_step: bool = False):
        """``actions`` float32 [E, B, K, 2] -> the returns f64 [E, B] of the sequences, each stepped from its environment's current
        state (``hwy_park_score``), and with ``per_step`` the reward f64 and the flags u8 [E, B, K] of every step."""
        a = np.ascontiguousarray(actions, np.float32)
        if a.ndim != 4 or a.shape[0] != self.E or a.shape[3] != 2:
            raise ValueError(f"actions must be [{self.E}, B, K, 2]")
        B, K = a.shape[1:3]
        ret = np.empty((self.E, B))
        sr, sf = (np.empty((self.E, B, K)), np.empty((self.E, B, K), np.uint8)) if per_step else (None, None)
        self._check(self.lib.hwy_park_score(self.h, B, K, float(gamma), _ptr(a), _ptr(ret), _ptr(sr), _ptr(sf)))
        return (ret, sr, sf) if per_step else ret

    def score_device(self, branches, k_steps, gamma, d_actions, d_ret, d_step_reward=None, d_step_flags=None):
        self._check(self.lib.hwy_park_score_device(self.h, int(branches), int(k_steps), float(gamma), d_actions, d_ret, d_step_reward, d_step_flags))

    def cem_plan(self, cem, init_mean=None, debug: bool = False) -> dict:
        """One search per environment (``hwy_park_cem_plan``): ``action`` f32 [E, 2], ``best_return``, ``best_sequence``, ``mean``,
        ``std``, and with ``debug`` every iteration's ``noise``, ``samples``, ``returns`` and ``elites``."""
        E, B, K, M, I = self.E, cem.population, cem.horizon, cem.elites, cem.iterations
        out = {"action": np.empty((E, 2), np.float32), "best_return": np.empty(E), "mean": np.empty((E, K, 2)), "std": np.empty((E, K, 2)),
               "best_sequence": np.empty((E, K, 2), np.float32)}
        dbg = {"noise": np.empty((I, E, B, K, 2)), "samples": np.empty((I, E, B, K, 2), np.float32), "returns": np.empty((I, E, B)),
               "elites": np.empty((I, E, M), np.int32)} if debug else {}
        im = None if init_mean is None else np.ascontiguousarray(init_mean, np.float64)
        self._check(self.lib.hwy_park_cem_plan(self.h, C.addressof(cem), _ptr(im), *(_ptr(out[k]) for k in ("action", "best_return", "mean", "std", "best_sequence")),
                                               *(_ptr(dbg.get(k)) for k in ("noise", "samples", "returns", "elites"))))
        return dict(out, **dbg)

    def cem_plan_device(self, cem, d_action, d_init_mean=None, d_best_return=None, d_mean=None, d_std=None, d_best_sequence=None,
                        d_noise=None, d_samples=None, d_returns=None, d_elites=None):
        self._check(self.lib.hwy_park_cem_plan_device(self.h, C.addressof(cem), d_init_mean, d_action, d_best_return, d_mean, d_std,
                                                      d_best_sequence, d_noise, d_samples, d_returns, d_elites))

    def mppi_plan(self, mppi, init_mean=None, debug: bool = False) -> dict:
        """One MPPI search per environment (``hwy_park_mppi_plan``): ``action`` f32 [E, 2], ``best_return``, ``mean``, ``weights_ess``,
        and with ``debug`` every iteration's ``noise``, ``samples``, ``returns``, ``weights`` and the ``mean_history``."""
        E, B, K, I = self.E, mppi.population, mppi.horizon, mppi.iterations
        out = {"action": np.empty((E, 2), np.float32), "best_return": np.empty(E), "mean": np.empty((E, K, 2)), "weights_ess": np.empty(E)}
        dbg = {"noise": np.empty((I, E, B, K, 2)), "samples": np.empty((I, E, B, K, 2), np.float32), "returns": np.empty((I, E, B)),
               "weights": np.empty((I, E, B)), "mean_history": np.empty((I + 1, E, K, 2))} if debug else {}
        im = None if init_mean is None else np.ascontiguousarray(init_mean, np.float64)
        self._check(self.lib.hwy_park_mppi_plan(self.h, C.addressof(mppi), _ptr(im), *(_ptr(out[k]) for k in ("action", "best_return", "mean", "weights_ess")),
                                                *(_ptr(dbg.get(k)) for k in ("noise", "samples", "returns", "weights", "mean_history"))))
        return dict(out, **dbg)

    def mppi_plan_device(self, mppi, d_action, d_init_mean=None, d_best_return=None, d_mean=None, d_weights_ess=None, d_noise=None,
                         d_samples=None, d_returns=None, d_weights=None, d_mean_history=None):
        self._check(self.lib.hwy_park_mppi_plan_device(self.h, C.addressof(mppi), d_init_mean, d_action, d_best_return, d_mean, d_weights_ess,
                                                       d_noise, d_samples, d_returns, d_weights, d_mean_history))


# ---- the lot and the host spawn (ParkingEnv._create_road / _create_vehicles on NumPy's generator) ----------------------------------
def spot_position(k):
    """Position of ``lane.position(4, 0)`` of spot k (lanes_dict order: ("a", "b", 0 .. 13), then ("b", "c", 0 .. 13))."""
    k = np.asarray(k)
    return 4.0 * (k % 14) - 26.0, np.where(k < 14, 14.0, -14.0)


def spot_heading(k):
    return np.where(np.asarray(k) < 14, np.pi / 2, -np.pi / 2)


def closest_spot(heading: float) -> int:
    """``RoadNetwork.get_closest_lane_index((0, 0), heading)`` (road.py:55-71, lane.py:132-143) over the 28 lanes."""
    ks = np.arange(SPOTS)
    x, _ = spot_position(ks)
    wrapped = ((heading - spot_heading(ks) + np.pi) % (2 * np.pi)) - np.pi
    dist = np.abs(np.where(ks < 14, x, -x)) + 0.0 + 10.0 + 1.0 * np.abs(wrapped)  # s = -10: max(s - 8, 0) + max(0 - s, 0)
    return int(np.argmin(dist))


def alloc_state(num_envs: int) -> dict:
    st = {k: np.zeros(num_envs) for k in EGO_FIELDS}
    st.update({k: np.zeros(num_envs, np.int32) for k in INT_FIELDS})
    st["order"] = np.zeros((num_envs, MAX_PARKED), np.uint8)
    st.update({k: np.zeros((num_envs, MAX_PARKED)) for k in PARKED_FIELDS})
    return st


def spawn_reference_stream(vehicles_count: int, rngs) -> dict:
    """The state ``ParkingEnv.reset`` leaves, one NumPy Generator per environment consumed in the reference's order: heading
    ``2 pi uniform()``, the ego's own spot out of the free list, ``choice`` for the goal, ``choice`` per parked vehicle."""
    st = alloc_state(len(rngs))
    for e, rng in enumerate(rngs):
        st["heading"][e] = 2.0 * np.pi * rng.uniform()
        free = list(range(SPOTS))
        free.remove(closest_spot(st["heading"][e]))
        st["goal"][e] = free.pop(int(rng.choice(np.arange(len(free)))))
        for _ in range(vehicles_count):
            if not free:
                continue
            k = free.pop(int(rng.choice(np.arange(len(free)))))
            st["order"][e, bin(int(st["occupied"][e])).count("1")] = k
            st["occupied"][e] |= 1 << k
    return st


def obs_dict(obs):
    """float32 [..., 3, 6] -> the reference's dict."""
    return {"observation": obs[..., 0, :], "achieved_goal": obs[..., 1, :], "desired_goal": obs[..., 2, :]}


def _spaces():
    if _gym is None:
        from .envs import _Box
        return {k: _Box((6,), np.float64) for k in ("desired_goal", "achieved_goal", "observation")}, _Box((2,), np.float32)
    box = lambda: _gym.spaces.Box(-np.inf, np.inf, (6,), np.float64)  # noqa: E731  (observation.py:507-531)
    return (_gym.spaces.Dict(dict(desired_goal=box(), achieved_goal=box(), observation=box())),
            _gym.spaces.Box(-1.0, 1.0, (2,), np.float32))


class BatchedParkingEnv:
    """E parallel ``parking-v0`` environments on one MI355X."""

    SCENARIO = "parking"
    CONFIG = {}

    def __init__(self, config: dict | None = None, num_envs: int = 1, device: int = 0, render_mode=None,
                 spawn_mode: str = "reference", autoreset: bool = False, stream: int | None = None, max_plan_bytes: int = 1 << 30):
        if render_mode is not None:
            raise NotImplementedError("rendering is outside the MI355X hot-path scope")
        if spawn_mode not in ("reference", "device"):
            raise ValueError("spawn_mode must be 'reference' (numpy PCG64 stream) or 'device' (Philox)")
        self.num_envs, self.device, self.spawn_mode, self.autoreset, self._stream = int(num_envs), device, spawn_mode, bool(autoreset), stream
        self.config = self.default_config()
        self.configure(config)
        self._engine = self._engine_key = None
        self._np_randoms = [None] * self.num_envs
        self.max_plan_bytes, self._plan_entropy, self._steps, self._cem_decisions = max_plan_bytes, 0, 0, 0
        self._define_spaces()

    @classmethod
    def default_config(cls) -> dict:
        cfg = parking_default_config()
        cfg.update(copy.deepcopy(cls.CONFIG))
        return cfg

    def configure(self, config: dict | None) -> None:
        for k, v in (config or {}).items():  # utils.update_config: nested dicts merge
            if isinstance(v, dict) and isinstance(self.config.get(k), dict):
                self.config[k] = {**self.config[k], **v}
            else:
                self.config[k] = v

    def _define_spaces(self):
        self._pcfg = make_park_config(self.config, self.num_envs, self.autoreset)
        self.single_observation_space, self.single_action_space = _spaces()
        self.observation_space, self.action_space = self.single_observation_space, self.single_action_space

    def _ensure_engine(self) -> ParkEngine:
        key = bytes(self._pcfg)
        if self._engine is None or key != self._engine_key:
            self.close()
            self._engine, self._engine_key = ParkEngine(self._pcfg, self.device, self._stream), key  # raises without a GPU
        return self._engine

    def close(self):
        if self._engine is not None:
            self._engine.close()
            self._engine = None

    def reset(self, *, seed=None, options: dict | None = None):
        if options and "config" in options:
            self.configure(options["config"])
        self._define_spaces()
        eng, E = self._ensure_engine(), self.num_envs
        seeds = [None] * E if seed is None else [int(seed) + e for e in range(E)] if np.ndim(seed) == 0 else list(seed)
        if len(seeds) != E:
            raise ValueError("one seed per env expected")
        for e, s in enumerate(seeds):
            if s is not None or self._np_randoms[e] is None:
                self._np_randoms[e] = np.random.Generator(np.random.PCG64(np.random.SeedSequence(s)))
        if self.spawn_mode == "reference":
            eng.set_state(spawn_reference_stream(self._pcfg.vehicles_count, self._np_randoms))
            obs = eng.observe()
        else:
            obs = eng.reset(seeds=[np.random.SeedSequence(s).generate_state(1, np.uint64)[0] if s is None else s for s in seeds])
        base = (int(np.random.SeedSequence(None).generate_state(1, np.uint64)[0] >> np.uint64(1)) if seeds[0] is None
                else int(seeds[0]) + 0x9E3779B9)
        eng.set_autoreset(self.autoreset, base)
        self._plan_entropy, self._steps, self._cem_decisions = base & (2 ** 64 - 1), 0, 0
        return obs_dict(obs), self._info(obs, np.zeros(E, np.uint8))

    def _info(self, obs, flags):
        return {"speed": np.hypot(obs[:, 0, 2] * self._pcfg.scales[2], obs[:, 0, 3] * self._pcfg.scales[3]).astype(np.float64),
                "crashed": (flags & S_CRASHED) != 0, "is_success": (flags & S_SUCCESS) != 0}

    def step(self, actions):
        """``actions`` float32 [E, 2] in [-1, 1] (throttle, steering; clipped) -> (obs dict, reward f64 [E], terminated, truncated, info)."""
        obs, reward, flags = self._ensure_engine().advance(np.asarray(actions, np.float32).reshape(1, self.num_envs, 2))
        self._steps += 1
        return obs_dict(obs), reward, (flags & S_TERMINATED) != 0, (flags & S_TRUNCATED) != 0, self._info(obs, flags)

    def rollout(self, actions):
        """K policy steps in one launch (action repeat, open-loop rollouts): ``actions`` float32 [K, E, 2] -> the observation of the
        last step and reward / terminated / truncated / is_success [K, E] of every step."""
        obs, _, _, sr, sf = self._ensure_engine().advance(actions, per_step=True)
        self._steps += len(sr)
        return obs_dict(obs), sr, (sf & S_TERMINATED) != 0, (sf & S_TRUNCATED) != 0, {"is_success": (sf & S_SUCCESS) != 0,
                                                                                        "crashed": (sf & S_CRASHED) != 0}

    def compute_reward(self, achieved_goal, desired_goal, info=None, p: float = 0.5):
        """``ParkingEnv.compute_reward`` of ``[M, 6]`` (or ``[6]``) arrays or CUDA tensors by the elementwise kernel, f64 out.  A
        tensor stays on the device: hindsight relabelling of a replay batch needs no host round trip."""
        if p != 0.5:
            raise NotImplementedError("parking: compute_reward with p != 0.5 is outside the scope of the device kernel")
        eng = self._ensure_engine()
        if type(achieved_goal).__module__.startswith("torch"):
            import torch
            a = achieved_goal.to(dtype=torch.float64).contiguous()
            d = torch.as_tensor(desired_goal, device=a.device).to(dtype=torch.float64).expand_as(a).contiguous()
            out = torch.empty(a.shape[:-1], dtype=torch.float64, device=a.device)
            torch.cuda.current_stream(a.device).synchronize()  # the inputs are ready before the handle's stream reads them
            eng.goal_reward_device(out.numel(), a.data_ptr(), d.data_ptr(), out.data_ptr())
            eng.sync()
            return out
        a = np.asarray(achieved_goal, np.float64)
        out = eng.goal_reward(a, np.broadcast_to(np.asarray(desired_goal, np.float64), a.shape))
        return out.reshape(a.shape[:-1]) if a.ndim > 1 else float(out[0])

    # ---- sampling MPC: csrc/hwy_park_cem.h, one launch per call ---------------------------------------------------------------------
    def _plan_fits(self):
        need = PLAN_BYTES_PER_ENV * self.num_envs
        if need > self.max_plan_bytes:
            raise MemoryError(f"parking: the candidates of {self.num_envs} environments keep {need} bytes of struck bodies on the device "
                              f"(max_plan_bytes = {self.max_plan_bytes})")

    def _sequences(self, actions):
        a, E = np.asarray(actions, np.float32), self.num_envs
        if a.ndim == 3:
            a = np.broadcast_to(a, (E, *a.shape))
        if a.ndim != 4 or a.shape[0] != E or a.shape[3] != 2 or a.shape[1] < 1 or a.shape[2] < 1:
            raise ValueError(f"action sequences must have shape [B, K, 2] or [{E}, B, K, 2]; got {np.shape(actions)}")
        if not np.isfinite(a).all():
            raise ValueError("action sequences must be finite")
        return np.ascontiguousarray(a)

    def _cem_setup(self, population, elites, iterations, horizon, gamma, init_std, min_std, alpha, seed):
        """The checks of ``plan_cem`` -- all before the engine is created -- and its ``hwy_cem_params``."""
        cem = park_cem_params(population, elites, iterations, horizon, gamma, init_std, min_std, alpha, self._plan_seed(seed))
        self._plan_fits()
        return cem

    def _plan_seed(self, seed):
        if seed is None:  # successive decisions draw different noise; an explicit seed is used as given
            seed = int(np.random.SeedSequence((self._plan_entropy, self._steps, self._cem_decisions)).generate_state(1, np.uint64)[0])
            self._cem_decisions += 1
        return seed

    def _mppi_setup(self, population, iterations, horizon, gamma, noise_std, temperature, beta, alpha, seed):
        """The checks of ``plan_mppi`` -- all before the engine is created -- and its ``hwy_park_mppi_params``."""
        mppi = park_mppi_params(population, iterations, horizon, gamma, noise_std, temperature, beta, alpha, self._plan_seed(seed))
        self._plan_fits()
        return mppi

    def _cem_init_mean(self, init_mean, K: int):
        if init_mean is None:
            return None
        m = np.asarray(init_mean, np.float64)
        if m.shape == (K, 2):
            m = np.broadcast_to(m, (self.num_envs, K, 2))
        if m.shape != (self.num_envs, K, 2):
            raise ValueError(f"init_mean must have shape ({K}, 2) or ({self.num_envs}, {K}, 2); got {m.shape}")
        if not np.isfinite(m).all():
            raise ValueError("init_mean must be finite")
        return np.ascontiguousarray(m)

    def score_sequences(self, actions, gamma: float = 1.0, return_details: bool = False):
        """B candidate sequences of K action pairs (float32 ``[B, K, 2]``, or ``[E, B, K, 2]``) are stepped from the CURRENT state with
        the true simulator, one candidate per lane of the environment's wavefront, and their discounted returns f64 [E, B] come
        back.  An episode that ends within a sequence is absorbing.  This environment is left exactly as it was.
        ``return_details``: also ``reward``, ``terminated``, ``truncated``, ``is_success``, ``crashed`` [E, B, K] of every step."""
        a = self._sequences(actions)
        park_cem_params(a.shape[1], 1, 1, a.shape[2], gamma, 0.0, 0.0, 1.0, 0)
        self._plan_fits()
        if not return_details:
            return self._ensure_engine().score(a, gamma)
        ret, sr, sf = self._ensure_engine().score(a, gamma, per_step=True)
        return ret, {"reward": sr, "terminated": (sf & S_TERMINATED) != 0, "truncated": (sf & S_TRUNCATED) != 0,
                     "is_success": (sf & S_SUCCESS) != 0, "crashed": (sf & S_CRASHED) != 0}

    def plan_cem(self, population: int = 64, elites: int = 8, iterations: int = 3, horizon: int = 8, gamma: float = 0.9,
                 init_std: float = 0.5, min_std: float = 0.05, alpha: float = 1.0, seed: int | None = None, init_mean=None,
                 return_details: bool = False, debug: bool = False):
        """Sampling MPC: the first action float32 [E, 2] of a cross-entropy-method search of every environment, the whole search in
        ONE launch (``hwy_park_cem_plan``; DESIGN.md "CEM on parking: one launch").  The signature and the rules are
        ``BatchedHighwayEnv.plan_cem``'s under parking's caps (population <= 256, horizon <= 32, population * horizon <= 4096,
        iterations <= 16).  ``seed=None``: derived from the seed of ``reset()``, the step count and the number of default-seed
        decisions since ``reset()``.  This environment is left exactly as it was.  ``return_details``: also ``best_return`` f64 [E],
        ``best_sequence`` f32 [E, K, 2], ``mean`` / ``std`` f64 [E, K, 2]; with ``debug`` also ``noise`` f64 / ``samples`` f32
        [I, E, B, K, 2], ``returns`` f64 [I, E, B] and ``elites`` int32 [I, E, M]."""
        cem = self._cem_setup(population, elites, iterations, horizon, gamma, init_std, min_std, alpha, seed)
        im = self._cem_init_mean(init_mean, cem.horizon)
        out = self._ensure_engine().cem_plan(cem, im, debug=debug)
        if not return_details:
            return out["action"]
        keys = ("best_return", "best_sequence", "mean", "std") + (("noise", "samples", "returns", "elites") if debug else ())
        return out["action"], {k: out[k] for k in keys}

    MPPI_DETAILS, MPPI_DEBUG = ("best_return", "mean", "weights_ess"), ("noise", "samples", "returns", "weights", "mean_history")

    def plan_mppi(self, population: int = 64, iterations: int = 3, horizon: int = 8, gamma: float = 0.9, noise_std: float = 0.5,
                  temperature: float = 0.1, beta: float = 0.0, alpha: float = 1.0, seed: int | None = None, init_mean=None,
                  return_details: bool = False, debug: bool = False):
        """Sampling MPC by MPPI (model-predictive path integral control): the first action float32 [E, 2] of the plan, the whole
        search of every environment in ONE launch (``hwy_park_mppi_plan``; DESIGN.md "MPPI on parking").  Every iteration draws
        ``population`` sequences ``clip(mean + noise_std * n, -1, 1)`` around the mean f64 [K, 2] (``init_mean`` or zeros), scores
        them with the true simulator and moves the mean to ``alpha`` times their average under the weights
        ``exp((return - best return) / temperature)`` plus ``1 - alpha`` times itself; the action is ``clip(mean[0], -1, 1)``.
        ``beta`` in [0, 1) colours the noise along the horizon, ``n[k] = beta n[k-1] + sqrt(1 - beta^2) z[k]`` (0: white); the white
        ``z`` and the caps are ``plan_cem``'s.  The default ``temperature`` of 0.1 is a guess: nobody has measured it.  Tune it by
        ``weights_ess``, the effective number of candidates the last update averaged.  ``seed=None``: ``plan_cem``'s rule.  This
        environment is left exactly as it was.  ``return_details``: also ``best_return`` f64 [E] (the highest return any candidate
        reached), ``mean`` f64 [E, K, 2], ``weights_ess`` f64 [E]; with ``debug`` also ``noise`` f64 / ``samples`` f32 [I, E, B, K, 2],
        ``returns`` / ``weights`` f64 [I, E, B] and ``mean_history`` f64 [I + 1, E, K, 2]."""
        mppi = self._mppi_setup(population, iterations, horizon, gamma, noise_std, temperature, beta, alpha, seed)
        im = self._cem_init_mean(init_mean, mppi.horizon)
        out = self._ensure_engine().mppi_plan(mppi, im, debug=debug)
        if not return_details:
            return out["action"]
        return out["action"], {k: out[k] for k in self.MPPI_DETAILS + (self.MPPI_DEBUG if debug else ())}

    def get_state(self) -> dict:
        return self._ensure_engine().get_state()

    def set_state(self, st: dict) -> None:
        self._ensure_engine().set_state(st)


class _SingleParkingMixin:
    """One environment with the reference's signatures: dict observation of float64 [6] rows, float reward, ``info["is_success"]``."""

    def __init__(self, config: dict | None = None, render_mode=None, device: int = 0):
        super().__init__(config, num_envs=1, device=device, render_mode=render_mode)

    def reset(self, *, seed=None, options=None):
        obs, info = super().reset(seed=seed, options=options)
        return self._one(obs), self._one_info(info)

    def step(self, action):
        obs, reward, term, trunc, info = super().step(np.asarray(action, np.float32).reshape(1, 2))
        return self._one(obs), float(reward[0]), bool(term[0]), bool(trunc[0]), dict(self._one_info(info), action=action)

    def score_sequences(self, actions, gamma: float = 1.0, return_details: bool = False):
        out = super().score_sequences(np.asarray(actions, np.float32)[None] if np.ndim(actions) == 3 else actions, gamma, return_details)
        return (out[0][0], {k: v[0] for k, v in out[1].items()}) if return_details else out[0]

    def plan_cem(self, *args, **kwargs):
        out = super().plan_cem(*args, **kwargs)
        if not isinstance(out, tuple):
            return out[0]
        return out[0][0], {k: (v[:, 0] if k in ("noise", "samples", "returns", "elites") else v[0]) for k, v in out[1].items()}

    def plan_mppi(self, *args, **kwargs):
        out = super().plan_mppi(*args, **kwargs)
        if not isinstance(out, tuple):
            return out[0]
        return out[0][0], {k: (v[:, 0] if k in self.MPPI_DEBUG else v[0]) for k, v in out[1].items()}

    @staticmethod
    def _one(obs):
        return {k: v[0].astype(np.float64) for k, v in obs.items()}

    @staticmethod
    def _one_info(info):
        return {"speed": float(info["speed"][0]), "crashed": bool(info["crashed"][0]), "is_success": bool(info["is_success"][0])}


class ParkingEnv(_SingleParkingMixin, BatchedParkingEnv, *_GYM_BASES):
    """Drop-in for ``highway_env.envs.parking_env.ParkingEnv`` (``parking-v0``)."""


class BatchedParkingEnvActionRepeat(BatchedParkingEnv):
    CONFIG = {"policy_frequency": 1, "duration": 20}


class ParkingEnvActionRepeat(_SingleParkingMixin, BatchedParkingEnvActionRepeat, *_GYM_BASES):
    """Drop-in for ``ParkingEnvActionRepeat`` (``parking-ActionRepeat-v0``)."""


class BatchedParkingEnvParkedVehicles(BatchedParkingEnv):
    CONFIG = {"vehicles_count": 10}


class ParkingEnvParkedVehicles(_SingleParkingMixin, BatchedParkingEnvParkedVehicles, *_GYM_BASES):
    """Drop-in for ``ParkingEnvParkedVehicles`` (``parking-parked-v0``)."""


REGISTRY = {
    "parking-v0": (ParkingEnv, BatchedParkingEnv),
    "parking-ActionRepeat-v0": (ParkingEnvActionRepeat, BatchedParkingEnvActionRepeat),
    "parking-parked-v0": (ParkingEnvParkedVehicles, BatchedParkingEnvParkedVehicles),
}
GYM_NAMESPACE = "highwayenv_amd"


def register_envs(namespace: str | None = GYM_NAMESPACE) -> list:
    """Register the three drop-ins with gymnasium (``envs.register_envs``'s rule: idempotent, [] without gymnasium)."""
    if _gym is None:
        return []
    from gymnasium.envs.registration import register, registry
    done = []
    for env_id, (single, _batched) in REGISTRY.items():
        full = f"{namespace}/{env_id}" if namespace else env_id
        if full not in registry:
            register(id=full, entry_point=f"{__name__}:{single.__name__}")
            done.append(full)
    return done


def is_parking_id(env) -> bool:
    return isinstance(env, str) and env.split("/", 1)[-1] in REGISTRY


def make(env_id: str, config: dict | None = None, **kwargs):
    return REGISTRY[env_id.split("/", 1)[-1]][0](config, **kwargs)


def make_vec(env_id: str, num_envs: int, config: dict | None = None, **kwargs):
    return REGISTRY[env_id.split("/", 1)[-1]][1](config, num_envs=num_envs, **kwargs)


class ParkingVectorEnv(_VecBase):
    """E parking environments behind the vector-env interface; what ``HighwayVectorEnv("parking-v0", E, ...)`` returns.
    ``Dict`` observations, ``Box(-1, 1, (2,), float32)`` actions, NextStep autoreset (or Disabled), ``info["is_success"]``.
    ``output="torch"``: actions may be CUDA tensors, observations, reward and flags are device tensors the kernel wrote (valid until
    the next step), one launch per step and no host round trip.  SameStep is not available on this front end."""

    def __init__(self, env="parking-v0", num_envs: int = 1, config: dict | None = None, autoreset_mode: str = "NextStep",
                 output: str = "numpy", device: int = 0, spawn_mode: str = "device", stream=None, max_plan_bytes: int = 1 << 30,
                 **kwargs):
        mode = str(getattr(autoreset_mode, "value", autoreset_mode)).lower().replace("_", "")
        if mode not in ("nextstep", "samestep", "disabled"):
            raise ValueError("autoreset_mode must be one of ('NextStep', 'SameStep', 'Disabled')")
        if mode == "samestep":
            raise NotImplementedError("parking: SameStep autoreset is not available (NextStep runs inside the advance kernel)")
        if output not in ("numpy", "torch"):
            raise ValueError("output must be 'numpy' or 'torch'")
        if kwargs:
            raise NotImplementedError(f"parking: {sorted(kwargs)} are not available on the parking scenario")
        self.autoreset_mode, self.output = ("NextStep" if mode == "nextstep" else "Disabled"), output
        self._torch = self._tstream = None
        if output == "torch":
            import torch
            self._torch = torch
            torch.cuda.set_device(device)
            if stream is None:
                cur = torch.cuda.current_stream(device)
                stream = cur if cur.cuda_stream else torch.cuda.Stream(device=device)
            self._tstream, stream = stream, stream.cuda_stream
        elif stream is not None:
            raise ValueError("stream= needs output='torch'")
        cls = REGISTRY[env.split("/", 1)[-1]][1] if isinstance(env, str) else env
        self.env = cls(config, num_envs=num_envs, device=device, spawn_mode=spawn_mode, autoreset=mode == "nextstep", stream=stream,
                       max_plan_bytes=max_plan_bytes)
        self.num_envs = self.env.num_envs
        self.single_observation_space, self.single_action_space = self.env.single_observation_space, self.env.single_action_space
        if _gym is not None:
            self.observation_space = _gym.vector.utils.batch_space(self.single_observation_space, self.num_envs)
            self.action_space = _gym.vector.utils.batch_space(self.single_action_space, self.num_envs)
        else:
            from .vector import _Batched
            self.observation_space = {k: _Batched(v, self.num_envs) for k, v in self.single_observation_space.items()}
            self.action_space = _Batched(self.single_action_space, self.num_envs)
        self.metadata, self.render_mode, self.closed, self._dev = {"autoreset_mode": self.autoreset_mode, "render_modes": []}, None, False, None

    def reset(self, *, seed=None, options=None):
        obs, info = self.env.reset(seed=seed, options=options)
        if self.output != "torch":
            return obs, info
        t, E = self._torch, self.num_envs
        dev = t.device("cuda", self.env.device)
        self._dev = {"obs": t.empty((E, 3, 6), dtype=t.float32, device=dev), "reward": t.empty(E, dtype=t.float64, device=dev),
                     "flags": t.empty(E, dtype=t.uint8, device=dev)}
        first = t.from_numpy(np.stack([obs["observation"], obs["achieved_goal"], obs["desired_goal"]], 1)).to(dev)
        return obs_dict(first), info

    def step(self, actions):
        if self.output != "torch":
            return self.env.step(actions)
        t, d = self._torch, self._dev
        a = (actions if isinstance(actions, t.Tensor) else t.as_tensor(np.asarray(actions, np.float32)))
        a = a.to(device=d["obs"].device, dtype=t.float32).reshape(self.num_envs, 2).contiguous()
        cur = t.cuda.current_stream()
        same = cur.cuda_stream == self._tstream.cuda_stream
        if not same:
            self._tstream.wait_stream(cur)
        self.env._engine.advance_device(1, a.data_ptr(), d["obs"].data_ptr(), d["reward"].data_ptr(), d["flags"].data_ptr())
        if not same:
            cur.wait_stream(self._tstream)
            a.record_stream(self._tstream)
        f = d["flags"]
        info = {"is_success": (f & S_SUCCESS) != 0, "crashed": (f & S_CRASHED) != 0}
        return obs_dict(d["obs"]), d["reward"], (f & S_TERMINATED) != 0, (f & S_TRUNCATED) != 0, info

    def _on_stream(self, enqueue, inputs=()):
        """Run ``enqueue()`` on the handle's stream, ordered against the current stream the way ``step`` is."""
        cur = self._torch.cuda.current_stream()
        same = cur.cuda_stream == self._tstream.cuda_stream
        if not same:
            self._tstream.wait_stream(cur)
        enqueue()
        if not same:
            cur.wait_stream(self._tstream)
            for x in inputs:
                x.record_stream(self._tstream)

    def score_sequences(self, actions, gamma: float = 1.0, return_details: bool = False):
        """``BatchedParkingEnv.score_sequences``.  ``output="torch"``: ``actions`` may be a device tensor (not validated: a non-finite
        pair keeps the stored controls), the returns and the details are device tensors, one launch and no host round trip."""
        if self.output != "torch":
            return self.env.score_sequences(actions, gamma, return_details)
        t, E, env = self._torch, self.num_envs, self.env
        if self._dev is None:
            raise RuntimeError("score_sequences() before reset()")
        dev = self._dev["obs"].device
        a = actions if isinstance(actions, t.Tensor) else t.from_numpy(env._sequences(actions))
        a = a.to(device=dev, dtype=t.float32)
        a = (a.unsqueeze(0).expand(E, *a.shape) if a.dim() == 3 else a).contiguous()
        if a.dim() != 4 or a.shape[0] != E or a.shape[3] != 2:
            raise ValueError(f"action sequences must have shape [B, K, 2] or [{E}, B, K, 2]; got {tuple(a.shape)}")
        B, K = int(a.shape[1]), int(a.shape[2])
        park_cem_params(B, 1, 1, K, gamma, 0.0, 0.0, 1.0, 0)
        env._plan_fits()
        ret = t.empty((E, B), dtype=t.float64, device=dev)
        sr = t.empty((E, B, K), dtype=t.float64, device=dev) if return_details else None
        sf = t.empty((E, B, K), dtype=t.uint8, device=dev) if return_details else None
        self._on_stream(lambda: env._engine.score_device(B, K, gamma, a.data_ptr(), ret.data_ptr(), sr.data_ptr() if return_details else None,
                                                         sf.data_ptr() if return_details else None), [a])
        if not return_details:
            return ret
        return ret, {"reward": sr, "terminated": (sf & S_TERMINATED) != 0, "truncated": (sf & S_TRUNCATED) != 0,
                     "is_success": (sf & S_SUCCESS) != 0, "crashed": (sf & S_CRASHED) != 0}

    def plan_cem(self, population: int = 64, elites: int = 8, iterations: int = 3, horizon: int = 8, gamma: float = 0.9,
                 init_std: float = 0.5, min_std: float = 0.05, alpha: float = 1.0, seed: int | None = None, init_mean=None,
                 return_details: bool = False, debug: bool = False):
        """``BatchedParkingEnv.plan_cem``.  ``output="torch"``: the device tensor the kernel wrote (and, with ``return_details``,
        device tensors of the details; valid until the next call of that horizon), ordered on the current stream like ``step`` --
        one ``hwy_park_cem_plan_device`` call, and ``env.step(env.plan_cem())`` never leaves the GPU.  ``init_mean``: a float64
        array or device tensor [K, 2] or [E, K, 2]; a device tensor is not validated."""
        if self.output != "torch":
            return self.env.plan_cem(population, elites, iterations, horizon, gamma, init_std, min_std, alpha, seed, init_mean,
                                     return_details=return_details, debug=debug)
        t, E, env = self._torch, self.num_envs, self.env
        cem = env._cem_setup(population, elites, iterations, horizon, gamma, init_std, min_std, alpha, seed)
        if self._dev is None:
            raise RuntimeError("plan_cem() before reset()")
        K, dev = cem.horizon, self._dev["obs"].device
        if ("cem", K) not in self._dev:
            self._dev["cem", K] = {"action": t.empty((E, 2), dtype=t.float32, device=dev), "best_return": t.empty(E, dtype=t.float64, device=dev),
                                   "mean": t.empty((E, K, 2), dtype=t.float64, device=dev), "std": t.empty((E, K, 2), dtype=t.float64, device=dev),
                                   "best_sequence": t.empty((E, K, 2), dtype=t.float32, device=dev)}
        d, dbg = self._dev["cem", K], {}
        if debug:  # (allocated per call: a test's door, not the hot path)
            shape = (cem.iterations, E, cem.population, K, 2)
            dbg = {"noise": t.empty(shape, dtype=t.float64, device=dev), "samples": t.empty(shape, dtype=t.float32, device=dev),
                   "returns": t.empty(shape[:3], dtype=t.float64, device=dev),
                   "elites": t.empty((cem.iterations, E, cem.elites), dtype=t.int32, device=dev)}
        im = None
        if init_mean is not None:
            if isinstance(init_mean, t.Tensor):
                im = init_mean.to(device=dev, dtype=t.float64)
                im = (im.unsqueeze(0).expand(E, K, 2) if im.dim() == 2 else im).reshape(E, K, 2).contiguous()
            else:
                im = t.from_numpy(env._cem_init_mean(init_mean, K)).to(dev)
        self._on_stream(lambda: env._engine.cem_plan_device(cem, d["action"].data_ptr(), None if im is None else im.data_ptr(),
                                                            *(d[k].data_ptr() for k in ("best_return", "mean", "std", "best_sequence")),
                                                            *(dbg[k].data_ptr() for k in ("noise", "samples", "returns", "elites") if debug)),
                        ([im] if im is not None else []) + list(dbg.values()))
        if not return_details:
            return d["action"]
        return d["action"], dict({k: d[k] for k in ("best_return", "best_sequence", "mean", "std")}, **dbg)

    def plan_mppi(self, population: int = 64, iterations: int = 3, horizon: int = 8, gamma: float = 0.9, noise_std: float = 0.5,
                  temperature: float = 0.1, beta: float = 0.0, alpha: float = 1.0, seed: int | None = None, init_mean=None,
                  return_details: bool = False, debug: bool = False):
        """``BatchedParkingEnv.plan_mppi`` (the default ``temperature`` is an untuned guess).  ``output="torch"``: the device tensor the
        kernel wrote (and, with ``return_details``, device tensors of the details; valid until the next call of that horizon),
        ordered on the current stream like ``step`` -- one ``hwy_park_mppi_plan_device`` call, and ``env.step(env.plan_mppi())``
        never leaves the GPU.  ``init_mean``: a float64 array or device tensor [K, 2] or [E, K, 2]; a device tensor is not validated."""
        if self.output != "torch":
            return self.env.plan_mppi(population, iterations, horizon, gamma, noise_std, temperature, beta, alpha, seed, init_mean,
                                      return_details=return_details, debug=debug)
        t, E, env = self._torch, self.num_envs, self.env
        mppi = env._mppi_setup(population, iterations, horizon, gamma, noise_std, temperature, beta, alpha, seed)
        if self._dev is None:
            raise RuntimeError("plan_mppi() before reset()")
        K, dev = mppi.horizon, self._dev["obs"].device
        if ("mppi", K) not in self._dev:
            self._dev["mppi", K] = {"action": t.empty((E, 2), dtype=t.float32, device=dev), "best_return": t.empty(E, dtype=t.float64, device=dev),
                                    "mean": t.empty((E, K, 2), dtype=t.float64, device=dev), "weights_ess": t.empty(E, dtype=t.float64, device=dev)}
        d, dbg = self._dev["mppi", K], {}
        if debug:  # (allocated per call: a test's door, not the hot path)
            shape = (mppi.iterations, E, mppi.population, K, 2)
            dbg = {"noise": t.empty(shape, dtype=t.float64, device=dev), "samples": t.empty(shape, dtype=t.float32, device=dev),
                   "returns": t.empty(shape[:3], dtype=t.float64, device=dev), "weights": t.empty(shape[:3], dtype=t.float64, device=dev),
                   "mean_history": t.empty((mppi.iterations + 1, E, K, 2), dtype=t.float64, device=dev)}
        im = None
        if init_mean is not None:
            if isinstance(init_mean, t.Tensor):
                im = init_mean.to(device=dev, dtype=t.float64)
                im = (im.unsqueeze(0).expand(E, K, 2) if im.dim() == 2 else im).reshape(E, K, 2).contiguous()
            else:
                im = t.from_numpy(env._cem_init_mean(init_mean, K)).to(dev)
        self._on_stream(lambda: env._engine.mppi_plan_device(mppi, d["action"].data_ptr(), None if im is None else im.data_ptr(),
                                                             *(d[k].data_ptr() for k in env.MPPI_DETAILS),
                                                             *(dbg[k].data_ptr() for k in env.MPPI_DEBUG if debug)),
                        ([im] if im is not None else []) + list(dbg.values()))
        if not return_details:
            return d["action"]
        return d["action"], dict({k: d[k] for k in env.MPPI_DETAILS}, **dbg)

    def step_async(self, actions):
        self._pending = actions

    def step_wait(self):
        return self.step(self._pending)

    def compute_reward(self, achieved_goal, desired_goal, info=None, p: float = 0.5):
        return self.env.compute_reward(achieved_goal, desired_goal, info, p)

    def close(self, **kwargs):
        if not self.closed:
            self.env.close()
            self.closed = True
