"""Host-side mirror of the reference's environment API for the accelerated path.

``BatchedHighwayEnv`` keeps the shape of ``AbstractEnv`` (highway_env/envs/common/abstract.py):
``default_config()`` / ``configure()`` / ``reset(seed=, options=)`` / ``step(action)`` / ``close()``,
same config dict keys as ``HighwayEnv.default_config`` (envs/highway_env.py:25-53) and the same
exceptions for what the reference rejects -- but steps E environments per call, and the body of
``_simulate`` + ``observe`` + ``_reward`` + ``_is_terminated`` + ``_is_truncated``
(abstract.py:259-317) is ONE C-ABI call into the HIP engine.

``HighwayEnv`` / ``HighwayEnvFast`` are the E == 1 drop-ins with the reference's unbatched return
types (obs ``(5,5) float32``, ``float`` reward, ``bool`` flags, ``info`` dict with
``speed/crashed/action/rewards``).
"""
from __future__ import annotations

import copy
import itertools

import numpy as np

from . import _abi, spawn
from . import finite_mdp as _finite_mdp
from . import merge as _merge
from . import intersection as _ix
from .engine import Engine

try:  # optional: only to expose real spaces when gymnasium is installed
    import gymnasium as _gym
except Exception:  # pragma: no cover - gymnasium is absent in the build image
    _gym = None


class _Discrete:
    def __init__(self, n):
        self.n, self.shape, self.dtype = n, (), np.int64

    def contains(self, x):
        return 0 <= int(x) < self.n

    def sample(self):
        return int(np.random.randint(self.n))


class _Tuple:
    """gymnasium.spaces.Tuple stand-in (MultiAgentAction.space, action.py:336-340): one sub-space per agent."""

    def __init__(self, spaces):
        self.spaces = tuple(spaces)

    def __len__(self):
        return len(self.spaces)

    def contains(self, x):
        return len(x) == len(self.spaces) and all(sp.contains(v) for sp, v in zip(self.spaces, x))

    def sample(self):
        return tuple(sp.sample() for sp in self.spaces)


class _Box:
    def __init__(self, shape, dtype=np.float32):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.low, self.high = (0, 255) if self.dtype == np.uint8 else (-np.inf, np.inf)

    def contains(self, x):
        return tuple(np.shape(x)) == self.shape


class VehicleView:
    """Read-only view of one vehicle of one env (reference: Vehicle / ControlledVehicle attributes)."""

    def __init__(self, st, e, i, behavior=None, direct=False):
        self.position = np.array([st["x"][e, i], st["y"][e, i]])
        self.heading = float(st["heading"][e, i])
        self.speed = float(st["speed"][e, i])
        self.lane_index = ("0", "1", int(st["lane"][e, i]))
        self.target_lane_index = ("0", "1", int(st["target_lane"][e, i]))
        self.target_speed = float(st["target_speed"][e, i])
        f = int(st["flags"][e, i])
        self.crashed = bool(f & _abi.F_CRASHED)
        self.check_collisions = bool(f & _abi.F_CHECK_COLLISIONS)
        self.controlled = bool(f & _abi.F_CONTROLLED)
        self.speed_index = int(st["speed_index"][e, i]) if self.controlled else None
        self.timer = None if self.controlled else float(st["timer"][e, i])
        self.DELTA = None if self.controlled else float(st["delta"][e, i])
        if behavior is not None and not self.controlled:  # LinearVehicle family (behavior.py:353-416)
            self.ACCELERATION_PARAMETERS = np.array(behavior[e, i, :3])
            self.STEERING_PARAMETERS = np.array(behavior[e, i, 3:])
        if direct and self.controlled:  # DiscreteAction: a plain Vehicle (action.py:132-134) has no target lane / speed / index
            del self.target_lane_index, self.target_speed, self.speed_index

    @property
    def velocity(self):
        return self.speed * np.array([np.cos(self.heading), np.sin(self.heading)])


class RoadView:
    def __init__(self, st, e, behavior=None, direct=False):
        self.vehicles = [VehicleView(st, e, i, behavior, direct) for i in range(st["x"].shape[1])]
        self.objects = []


class BatchedHighwayEnv:
    """E parallel ``highway-v0``-family environments on one MI355X."""

    #: ``HighwayEnvFast`` semantics (ego-only collision checks, highway_env.py:177-182)
    FAST = False
    #: "highway" | "merge" | "merge-generic" (``_abi.make_config``)
    SCENARIO = "highway"
    PERCEPTION_DISTANCE = 5.0 * 40.0
    #: the HIP engine; tests substitute the CPU emulation of the same kernel source
    _engine_factory = staticmethod(lambda cfg, device, stream: Engine(cfg, device=device, stream=stream))

    def __init__(self, config: dict | None = None, num_envs: int = 1, device: int = 0, render_mode=None,
                 spawn_mode: str = "reference", autoreset: bool = False, stream: int | None = None):
        if render_mode is not None:
            raise NotImplementedError("rendering is outside the MI355X hot-path scope")
        if spawn_mode not in ("reference", "device"):
            raise ValueError("spawn_mode must be 'reference' (numpy PCG64 stream) or 'device' (Philox)")
        self.num_envs = int(num_envs)
        self.device = device
        self.spawn_mode = spawn_mode
        self.autoreset = bool(autoreset)
        self._stream = stream
        self.config = self.default_config()
        self.configure(config)
        self._engine = None
        self._engine_key = None
        self._np_randoms = [None] * self.num_envs  # per-env Generator == reference env.np_random
        self.time = np.zeros(self.num_envs)
        self.steps = 0
        self._cem_decisions = 0  # plan_cem(seed=None) calls since reset()
        self._define_spaces()

    @property
    def np_random(self):
        """Batched classes: the list of per-environment Generators (env e's == the reference env's ``np_random`` after
        ``reset(seed=seeds[e])``).  The single-environment drop-ins return THE Generator (``_SingleEnvMixin``)."""
        return self._np_randoms

    @np_random.setter
    def np_random(self, value):
        self._np_randoms = list(value) if isinstance(value, (list, tuple)) else [value] * self.num_envs

    # ---- config (abstract.py:101-144) ------------------------------------------------------
    @classmethod
    def default_config(cls) -> dict:
        return _abi.highway_fast_default_config() if cls.FAST else _abi.highway_default_config()

    def configure(self, config: dict | None) -> None:
        if config:
            self.config.update(config)

    def _define_spaces(self):
        hc = _abi.make_config(self.config, self.num_envs, fast=self.FAST, scenario=self.SCENARIO)
        self._hcfg = hc
        A = hc.num_agents
        self.single_observation_shape = _abi.obs_shape(hc) if A == 1 else (A, *_abi.obs_shape(hc))
        if _gym is not None:
            self.single_action_space = _gym.spaces.Discrete(_abi.num_actions(hc))  # len(self.actions), action.py:252-253
            image = bool(hc.flags & _abi.C_GRID_IMAGE)  # observation.py:330-331: Box(0, 255, uint8)
            self.single_observation_space = (_gym.spaces.Box(0, 255, self.single_observation_shape, np.uint8) if image else
                                             _gym.spaces.Box(-np.inf, np.inf, self.single_observation_shape, np.float32))
        else:
            self.single_action_space = _Discrete(_abi.num_actions(hc))
            self.single_observation_space = _Box(self.single_observation_shape, np.uint8 if hc.flags & _abi.C_GRID_IMAGE else np.float32)
        if hc.obs_type == _abi.OBS_LIDAR:
            # LidarObservation.space (observation.py:698-700): Box(-high, high, (cells, 2), float32), high = 1 if normalize else
            # maximum_range (MultiAgentObservation: one such space per agent, stacked here like the observation)
            high = 1.0 if hc.lidar_normalize else float(hc.lidar_max_range)
            if _gym is not None:
                self.single_observation_space = _gym.spaces.Box(-high, high, self.single_observation_shape, np.float32)
            else:
                self.single_observation_space.low, self.single_observation_space.high = -high, high
        self.action_space, self.observation_space = self.single_action_space, self.single_observation_space

    def _ensure_engine(self):
        key = bytes(self._hcfg)
        if self._engine is None or key != self._engine_key:
            if self._engine is not None:
                self._engine.close()
            self._engine = self._engine_factory(self._hcfg, self.device, self._stream)  # raises without a GPU
            self._engine_key = key
        return self._engine

    # ---- reset (abstract.py:219-249) -----------------------------------------------------------
    def reset(self, *, seed=None, options: dict | None = None):
        if options and "config" in options:
            self.configure(options["config"])
        self._define_spaces()
        eng = self._ensure_engine()
        E = self.num_envs
        if seed is None:
            seeds = [None] * E
        elif np.ndim(seed) == 0:
            seeds = [int(seed) + e for e in range(E)]  # gymnasium vector-env convention
        else:
            seeds = list(seed)
            if len(seeds) != E:
                raise ValueError("one seed per env expected")
        for e, s in enumerate(seeds):
            if s is not None or self._np_randoms[e] is None:
                # gymnasium.utils.seeding.np_random(seed): Generator(PCG64(SeedSequence(seed)))
                self._np_randoms[e] = np.random.Generator(np.random.PCG64(np.random.SeedSequence(s)))
        if self.spawn_mode == "reference":
            st0 = self._spawn_reference(self._np_randoms)
            eng.set_state(st0)
            if "behavior" in st0:  # LinearVehicle-family traffic: the parameters randomize_behavior drew
                eng.set_behavior(st0["behavior"])
            obs = eng.observe()
        else:
            sd = np.array([np.random.SeedSequence(s).generate_state(1, np.uint64)[0] if s is None else s
                           for s in seeds], np.uint64)
            obs = eng.reset(seeds=sd, **self._device_spawn_args())
        # auto-reset episodes: derived from the given seed (reproducible), or as unseeded as the first episode when
        # seed is None (fresh OS entropy -- otherwise every seed=None worker would replay the same later episodes)
        if seeds[0] is None:
            base_seed = int(np.random.SeedSequence(None).generate_state(1, np.uint64)[0] >> np.uint64(1))
        else:
            base_seed = int(seeds[0]) + 0x9E3779B9
        eng.set_autoreset(self.autoreset, base_seed=base_seed, **self._device_spawn_args())
        # SameStep re-spawns (reset_done): their own stream, keyed by the user's seed (reproducible; fresh entropy for seed=None)
        # and restarted by every reset() -- a SeedSequence child, so that no (seed, env, episode) meets a first-episode seed s + e
        self._same_step_entropy = int(base_seed)
        self._episodes = np.zeros(E, np.uint64)
        self.time[:] = 0
        self.steps = 0
        self._cem_decisions = 0
        st = eng.get_state()
        rows, ego = np.arange(E), self._ego_slots(st)
        info = {"speed": st["speed"][rows, ego].copy(), "crashed": (st["flags"][rows, ego] & _abi.F_CRASHED) != 0,
                "action": None}
        return self._shape_obs(obs), info

    def reset_done(self, mask) -> np.ndarray:
        """Re-spawn the environments of ``mask`` [E] on the device NOW (the "SameStep" autoreset of a vector env: the step that
        ended an episode also returns the next episode's first observation) and return their observations [k, ...].  Seeds:
        hashed from (the seed given to reset(), env, episode number) -- reproducible per user seed, different between user
        seeds, restarted by reset() (``spawn_mode="device"`` only)."""
        if self.spawn_mode != "device":
            raise NotImplementedError("reset_done (SameStep autoreset) needs spawn_mode='device'")
        mask = np.asarray(mask, bool)
        if self._engine is None or getattr(self, "_episodes", None) is None or len(self._episodes) != self.num_envs:
            raise RuntimeError("reset_done before reset()")
        self._episodes[mask] += np.uint64(1)
        # seed of (env e, episode k) = SeedSequence(entropy of this reset(), spawn_key=(0x5A3E, e, k)): hashed, so two user seeds
        # never replay each other's later episodes and no later episode repeats a first one (seed + e)
        seeds = np.zeros(self.num_envs, np.uint64)
        for e in np.flatnonzero(mask):
            seeds[e] = np.random.SeedSequence(self._same_step_entropy, spawn_key=(0x5A3E, int(e), int(self._episodes[e]))
                                              ).generate_state(1, np.uint64)[0]
        obs = self._engine.reset(seeds=seeds, mask=mask.astype(np.uint8), **self._device_spawn_args())
        self.time[mask] = 0
        return self._shape_obs(obs)[mask]

    def _ego_slots(self, st) -> np.ndarray:
        """Slot of the (first) controlled vehicle of every env."""
        return np.full(self.num_envs, self._hcfg.agent_index[0])

    def _spawn_reference(self, generators) -> dict:
        """``_create_vehicles`` replayed on each env's numpy Generator (highway_env.py:72-98)."""
        cfg = self.config
        return spawn.spawn_reference_stream(self._hcfg, generators, cfg["ego_spacing"], cfg["vehicles_density"],
                                            cfg["initial_lane_id"])

    def _device_spawn_args(self) -> dict:
        cfg = self.config
        lane_id = cfg["initial_lane_id"]
        return {"ego_spacing": cfg["ego_spacing"], "vehicles_density": cfg["vehicles_density"],
                "initial_lane_id": -1 if lane_id is None else lane_id}

    # ---- step (abstract.py:259-285) ---------------------------------------------------------------
    def step(self, action):
        if self._engine is None:
            # the reference raises NotImplementedError when road/vehicle are unset (abstract.py:269-272)
            raise NotImplementedError("The road and vehicle must be initialized in the environment implementation")
        E, A = self.num_envs, self._hcfg.num_agents
        acts = np.asarray(action)
        # accepted shapes: scalar (every env, every agent), (E,) = one action per env (single-agent envs; with A > 1 it
        # drives every agent of env e, never "agent a of every env"), (E, A) / (E*A,) as is
        if acts.ndim == 0:
            acts = np.broadcast_to(acts, (E, A))
        elif acts.shape == (E,) and not (A > 1 and E == 1):
            acts = np.broadcast_to(acts[:, None], (E, A))
        elif acts.shape == (E, A) or (acts.ndim == 1 and acts.size == E * A):
            acts = acts.reshape(E, A)
        else:
            raise ValueError(f"action must be a scalar, shape ({E},) or shape ({E}, {A}); got {acts.shape}")
        # a bad action id: KeyError (DiscreteMetaAction, action.py:260) / IndexError (DiscreteAction, action.py:195)
        obs, reward, term, trunc, info = self._engine.step(acts.astype(np.int32))
        self.time += 1 / self.config["policy_frequency"]
        self.steps += self._hcfg.frames_per_step
        out_info = {"speed": info["speed"][:, 0], "crashed": info["crashed"][:, 0], "action": acts if A > 1 else acts[:, 0]}
        self._agents_step = (reward, info)  # per-agent [E, A] results of this step (scenario subclasses build their info from them)
        if A > 1:
            out_info["agents_rewards"] = reward
            out_info["agents_speed"], out_info["agents_crashed"] = info["speed"], info["crashed"]
        return self._shape_obs(obs), reward[:, 0], term, trunc, out_info

    # ---- continuous throttle and steering (ContinuousAction.act, action.py:136-163) ----------------------------------------------
    def continuous_params(self) -> "_abi.HwyContinuousParams":
        """The ``ContinuousAction`` behind this env's ``DiscreteAction`` config (same vehicle class, same ``acceleration_range`` /
        ``steering_range`` / ``longitudinal`` / ``lateral`` / ``clip`` keys: ``DiscreteAction`` inherits them, action.py:165-188).
        NotImplementedError on a ``DiscreteMetaAction`` ego (an MDPVehicle follows lanes and speeds, not a throttle) and for
        ``clip: False``."""
        if self._hcfg.ego_control != _abi.EGO_DIRECT:
            raise NotImplementedError("step_continuous needs a plain-Vehicle ego: configure the env with {'type': 'DiscreteAction'} "
                                      "(a DiscreteMetaAction ego is an MDPVehicle)")
        act = self.config["action"]
        return _abi.continuous_params(act["action_config"] if act["type"] == "MultiAgentAction" else act)

    def continuous_action_space(self):
        """``ContinuousAction.space()`` (action.py:113-118): ``Box(-1, 1, (size,), float32)``, size 2 with both axes (throttle,
        steering), 1 with one; its stand-in without gymnasium."""
        size = self.continuous_params().size
        if _gym is not None:
            return _gym.spaces.Box(-1.0, 1.0, (size,), np.float32)
        box = _Box((size,), np.float32)
        box.low, box.high = -1.0, 1.0
        return box

    def _continuous_actions(self, action, size: int) -> np.ndarray:
        """``action`` as float32 [E, A, size]: shape (size,) drives every agent of every env, (E, size) every agent of env e,
        (E, A, size) is taken as is.  Cast to float32: a float64 array is ROUNDED first."""
        E, A = self.num_envs, self._hcfg.num_agents
        a = np.asarray(action, np.float32)
        if a.shape == (size,):
            a = np.broadcast_to(a, (E, A, size))
        elif a.shape == (E, size):
            a = np.broadcast_to(a[:, None, :], (E, A, size))
        elif a.shape != (E, A, size):
            raise ValueError(f"a continuous action must have shape ({size},), ({E}, {size}) or ({E}, {A}, {size}); got {a.shape}")
        return np.ascontiguousarray(a)

    def step_continuous(self, action):
        """``step`` with the reference's ``ContinuousAction`` in place of the action ids: ``action`` in [-1, 1]^size per agent
        (size 2: throttle, steering; 1 with ``longitudinal`` or ``lateral`` off; shapes (size,), (E, size), (E, A, size)) is
        clipped and mapped onto ``acceleration_range`` / ``steering_range`` on the device (csrc/hwy_act.h) exactly as
        ``ContinuousAction.get_action`` maps a float32 action, then the engine's own step runs on the stored pair.  The action
        is cast to float32; a float64 array is rounded to float32 FIRST -- the reference's ``Box(-1, 1, (size,), float32)``
        would not contain it either.  ``info["action"]`` echoes the float32 array.  ValueError for a NaN or an infinity,
        NotImplementedError on a ``DiscreteMetaAction`` ego and for ``clip: False``."""
        params = self.continuous_params()
        if self._engine is None:
            raise NotImplementedError("The road and vehicle must be initialized in the environment implementation")
        A = self._hcfg.num_agents
        acts = self._continuous_actions(action, params.size)
        obs, reward, term, trunc, info = self._engine.step_continuous(params, acts)
        self.time += 1 / self.config["policy_frequency"]
        self.steps += self._hcfg.frames_per_step
        out_info = {"speed": info["speed"][:, 0], "crashed": info["crashed"][:, 0], "action": acts if A > 1 else acts[:, 0]}
        self._agents_step = (reward, info)
        if A > 1:
            out_info["agents_rewards"] = reward
            out_info["agents_speed"], out_info["agents_crashed"] = info["speed"], info["crashed"]
        return self._shape_obs(obs), reward[:, 0], term, trunc, out_info

    def _shape_obs(self, obs):
        # KinematicObservation(order="shuffled") (observation.py:273-274): `self.env.np_random.shuffle(obs[1:])` after every
        # observe(), agent by agent -- the engine returned the rows in list order (HWY_C_OBS_UNSORTED), the shuffle draws
        # from each environment's own generator like the reference's (same stream as its spawn in spawn_mode="reference")
        if self._hcfg.flags & _abi.C_OBS_UNSORTED:
            obs = np.array(obs, copy=True)
            for e in range(self.num_envs):
                if self._np_randoms[e] is None:
                    self._np_randoms[e] = np.random.Generator(np.random.PCG64(np.random.SeedSequence(None)))
                for a in range(self._hcfg.num_agents):
                    self._np_randoms[e].shuffle(obs[e, a, 1:])
        if self._hcfg.flags & _abi.C_GRID_IMAGE:  # OccupancyGrid(as_image=True): the engine wrote the uint8 values as f32
            obs = obs.astype(np.uint8)
        return obs[:, 0] if self._hcfg.num_agents == 1 else obs

    # ---- inspection --------------------------------------------------------------------------------
    def get_state(self) -> dict:
        return self._engine.get_state()

    def set_state(self, st: dict) -> None:
        self._ensure_engine().set_state(st)

    def road(self, env_index: int = 0) -> RoadView:
        behavior = self._engine.get_behavior() if self._hcfg.traffic_model == _abi.TRAFFIC_LINEAR else None
        return RoadView(self._engine.get_state(), env_index, behavior, self._hcfg.ego_control == _abi.EGO_DIRECT)

    def rewards(self, env_index: int = 0) -> dict:
        """HighwayEnv._rewards (highway_env.py:122-139) of one env, from the device state."""
        st = self._engine.get_state()
        c, i = self._hcfg, self._hcfg.agent_index[0]
        x, y, h, v = (st[k][env_index, i] for k in ("x", "y", "heading", "speed"))
        lane, tgt = int(st["lane"][env_index, i]), int(st["target_lane"][env_index, i])
        if c.ego_control == _abi.EGO_DIRECT:  # a plain Vehicle: lane_index[2] (highway_env.py:122-126)
            tgt = lane
        fs = v * np.cos(h)
        r0, r1 = self.config["reward_speed_range"]
        scaled = 0 + (fs - r0) * (1 - 0) / (r1 - r0)
        on_road = abs(y - lane * c.lane_width) <= c.lane_width / 2 and -5 <= x < c.road_length + 5
        return {"collision_reward": float(bool(st["flags"][env_index, i] & _abi.F_CRASHED)),
                "right_lane_reward": tgt / max(c.lanes_count - 1, 1),
                "high_speed_reward": float(np.clip(scaled, 0, 1)),
                "on_road_reward": float(on_road)}

    # ---- get_available_actions (abstract.py:357 -> action.py:262-298) ---------------------------------------------------
    def get_available_actions(self) -> np.ndarray:
        """``AbstractEnv.get_available_actions`` of every controlled vehicle of every environment, computed on the device
        (csrc/hwy_mask.h): bool [E, n_ids] ([E, A, n_ids] for several agents), column i = action id i of the action table is
        available now.  NotImplementedError with ``DiscreteAction``, like the reference's ``ActionType``."""
        if self._hcfg.ego_control != _abi.EGO_META:
            raise NotImplementedError("get_available_actions needs a DiscreteMetaAction ego")
        if self._engine is None:
            raise NotImplementedError("The road and vehicle must be initialized in the environment implementation")
        mask = self._engine.action_mask()
        return mask[:, 0] if self._hcfg.num_agents == 1 else mask

    # ---- to_finite_mdp (abstract.py:452-453 -> envs/common/finite_mdp.py) -----------------------------------------
    def _ttc_params(self, horizon, time_quantization=None, gamma=1.0):
        _abi.check_finite_mdp_scope(self._hcfg)  # NotImplementedError outside the highway scenario / the five meta-actions
        params = _abi.ttc_params(self.config, horizon, time_quantization, gamma)
        if self._engine is None:
            raise NotImplementedError("The road and vehicle must be initialized in the environment implementation")
        return params

    def ttc_grid(self, horizon: float = 10.0, time_quantization: float | None = None) -> np.ndarray:
        """``compute_ttc_grid`` (finite_mdp.py:104-163) of every controlled vehicle of every environment, computed on the device:
        f64 [E, A, V, L, T] (speeds x lanes x time steps; 0, 0.5 or 1).  ``time_quantization`` defaults to
        ``1 / policy_frequency`` like ``to_finite_mdp``."""
        params = self._ttc_params(horizon, time_quantization)
        return self._engine.ttc_grid(params).astype(np.float64)

    def to_finite_mdp(self, env_index: int = 0, horizon: float = 10.0) -> "_finite_mdp.FiniteMDP":
        """``AbstractEnv.to_finite_mdp`` of environment ``env_index`` for its first controlled vehicle (``env.vehicle``): the grid
        comes from the device, the tables are built on the host (``highwayenv_amd.finite_mdp``).  The result carries the
        attributes the reference gives ``finite_mdp.mdp.DeterministicMDP``: ``transition``, ``reward``, ``terminal``, ``state``,
        ``original_shape``.  (The device computes the grid of every environment in one launch; one row of it is converted.)"""
        params = self._ttc_params(horizon, None)
        grid = self._engine.ttc_grid(params)[env_index, 0].astype(np.float64)
        st = self._engine.get_state()
        i = int(self._ego_slots(st)[env_index])
        return _finite_mdp.build(grid, int(st["speed_index"][env_index, i]), int(st["lane"][env_index, i]), self.config)

    def plan_finite_mdp(self, gamma: float = 1.0, horizon: float = 10.0, return_q: bool = False):
        """The reference's value-iteration policy on ``to_finite_mdp()`` for every controlled vehicle, solved on the device:
        meta-action ids int32 [E] ([E, A] for several agents); with ``return_q`` also Q(state, .) f64 [E(, A), 5]."""
        params = self._ttc_params(horizon, None, gamma)
        action, q, _ = self._engine.mdp_plan(params, return_q=return_q)
        if self._hcfg.num_agents == 1:
            action, q = action[:, 0], (q[:, 0] if q is not None else None)
        return (action, q) if return_q else action

    # ---- TimeToCollisionObservation (envs/common/observation.py:115-152), through a door of its own ------------------------------
    def _ttc_obs_params(self, horizon, need_engine: bool = True):
        _abi.check_ttc_observation_scope(self._hcfg)  # NotImplementedError off the highway / with a DiscreteAction ego
        params = _abi.ttc_params(self.config, horizon, None)  # time step 1 / policy_frequency (observation.py:131)
        if need_engine and self._engine is None:
            raise NotImplementedError("The road and vehicle must be initialized in the environment implementation")
        return params

    def ttc_observation(self, horizon: float = 10.0) -> np.ndarray:
        """``TimeToCollisionObservation(env, horizon).observe()`` of every controlled vehicle of every environment, computed on the
        device by a kernel of its own (csrc/hwy_collision_obs.h): float32 [E, 3, 3, T] ([E, A, 3, 3, T] for several agents), axes
        speeds ``speed_index - 1 .. + 1`` (clamped) x lanes ``lane - 1 .. + 1`` (1.0 off the road) x ``T = int(horizon *
        policy_frequency)`` time steps; values 0, 0.5 or 1.  The config type ``{"type": "TimeToCollision"}`` stays rejected: the
        env keeps its configured observation and hands this one out next to it."""
        params = self._ttc_obs_params(horizon)
        obs = self._engine.ttc_observe(params)
        return obs[:, 0] if self._hcfg.num_agents == 1 else obs

    def ttc_observation_space(self, horizon: float = 10.0):
        """``TimeToCollisionObservation.space()``: ``Box(0, 1, (3, 3, T), float32)``; several agents: a tuple of them
        (MultiAgentObservation.space, observation.py:598-601)."""
        shape = _abi.ttc_obs_shape(self._ttc_obs_params(horizon, need_engine=False))
        if _gym is not None:
            one = lambda: _gym.spaces.Box(0, 1, shape, np.float32)  # noqa: E731
            tup = _gym.spaces.Tuple
        else:
            def one():
                box = _Box(shape, np.float32)
                box.low, box.high = 0, 1
                return box
            tup = _Tuple
        A = self._hcfg.num_agents
        return one() if A == 1 else tup([one() for _ in range(A)])

    # ---- LidarObservation (envs/common/observation.py:678-769), through a door of its own -------------------------------------------
    def lidar_observation(self, cells: int = 16, maximum_range: float = 60.0, normalize: bool = True) -> np.ndarray:
        """``LidarObservation(env, cells, maximum_range, normalize).observe()`` of every controlled vehicle of every environment,
        traced on the device by a kernel of its own (csrc/hwy_lidar_door.h) on EVERY scenario family, next to the configured
        observation type: float32 [E, cells, 2] ([E, A, cells, 2] for several agents), (distance, relative radial speed) per cell,
        up to 256 cells; a merge scenario's ``Obstacle`` is traced as the 2 m x 2 m object it is.  The config type
        ``{"type": "LidarObservation"}`` stays what it was (highway ids, up to 64 cells).

        Intersection: the reference's ``step()`` observes BEFORE ``_clear_vehicles()`` / ``_spawn_vehicle()``
        (intersection_env.py:136-140); this call sees the vehicle list AFTER them.  It is what
        ``env.unwrapped.observation_type.observe()`` returns when called after ``step()`` -- not the value ``step()`` returned."""
        params = _abi.lidar_door_params(cells, maximum_range, normalize)
        if self._engine is None:
            raise NotImplementedError("The road and vehicle must be initialized in the environment implementation")
        obs = self._engine.lidar_observe(params)
        return obs[:, 0] if self._hcfg.num_agents == 1 else obs

    def lidar_observation_space(self, cells: int = 16, maximum_range: float = 60.0, normalize: bool = True):
        """``LidarObservation.space()``: ``Box(-high, high, (cells, 2), float32)`` with ``high`` 1 if normalised, else
        ``maximum_range``; several agents: a tuple of them (MultiAgentObservation.space, observation.py:598-601)."""
        params = _abi.lidar_door_params(cells, maximum_range, normalize)
        shape, high = _abi.lidar_door_shape(params), (1 if params.normalize else params.maximum_range)
        if _gym is not None:
            one = lambda: _gym.spaces.Box(-high, high, shape, np.float32)  # noqa: E731
            tup = _gym.spaces.Tuple
        else:
            def one():
                box = _Box(shape, np.float32)
                box.low, box.high = -high, high
                return box
            tup = _Tuple
        A = self._hcfg.num_agents
        return one() if A == 1 else tup([one() for _ in range(A)])

    # ---- fork / score_sequences / plan_lookahead: AbstractEnv.__deepcopy__ + step on the copy (abstract.py:455) ------------------
    def _lookahead_scope(self, what: str):
        if self._hcfg.scenario != _abi.SCENARIO_HIGHWAY:
            raise NotImplementedError(f"{what} is in the MI355X hot-path scope on the highway scenario only")
        if self._engine is None:
            raise NotImplementedError("The road and vehicle must be initialized in the environment implementation")

    def fork(self, branches: int = 1, source=None) -> "BatchedHighwayEnv":
        """``copy.deepcopy(env)`` for every environment at once, on the device: an environment of ``E * branches`` environments
        with this one's config, auto-reset off, already reset -- environment ``e * branches + b`` is copy ``b`` of environment
        ``e`` (``hwy_fork_device``: the state never visits the host).  ``source``: int array [E'] of parent indices (repeated,
        out of order, some omitted); the child then holds ``E' * branches`` environments, copies of ``source[j // branches]``.
        The child is cached on the parent per (num_envs, branches) and OVERWRITTEN by the next such fork.  An environment that
        awaits its NextStep re-spawn is forked as it stands: stepping the copy continues the ended episode, which is what
        stepping the reference after ``done`` gives."""
        self._lookahead_scope("fork")
        B = int(branches)
        if B < 1:
            raise ValueError("branches must be >= 1")
        idx = None
        if source is not None:
            idx = np.asarray(source)
            if idx.ndim != 1 or idx.size < 1 or not np.issubdtype(idx.dtype, np.integer):
                raise ValueError("source must be a non-empty 1-D integer array of parent indices")
            if ((idx < 0) | (idx >= self.num_envs)).any():
                raise ValueError(f"source holds an index outside [0, {self.num_envs})")
            idx = np.repeat(idx.astype(np.int32), B)
        n = (self.num_envs if idx is None else idx.size // B) * B
        self._lookahead_fits(n, 0)
        child = self._fork_child((n, B), n, "fork")
        child._engine.fork_from(self._engine, B, idx)
        if self._stream is None:  # each engine has a stream of its own: the copy is complete before the parent is written again
            child._engine.sync()
        src = np.arange(n) // B if idx is None else idx
        child._np_randoms = [self._np_randoms[e] for e in src]
        child.time = self.time[src].copy()
        child.steps = self.steps
        return child

    def _fork_child(self, key, n: int, what: str) -> "BatchedHighwayEnv":
        """The cached child environment of ``n`` environments under ``key``: this one's config, auto-reset off, its engine built."""
        forks = self.__dict__.setdefault("_forks", {})
        child = forks.get(key)
        if child is None or child._parent_key != self._engine_key or child._engine is None:
            if child is not None:
                child.close()
            cls = BatchedHighwayEnvFast if self.FAST else BatchedHighwayEnv
            child = cls(_copy_config(self.config), num_envs=n, device=self.device, spawn_mode=self.spawn_mode, autoreset=False,
                        stream=self._stream)
            child._engine_factory = self._engine_factory
            child._define_spaces()
            try:
                child._ensure_engine()
            except Exception as exc:  # the device has no room for the branches
                if "memory" in str(exc).lower():
                    raise ValueError(f"{what}: {n} environments need {_abi.fork_bytes(self._hcfg, n, 0)} bytes of device memory, "
                                     f"which the device does not have") from exc
                raise
            child._engine.set_autoreset(False)
            child._parent_key = self._engine_key
            forks[key] = child
        return child

    def _lookahead_fits(self, n: int, k_steps: int):
        need = _abi.fork_bytes(self._hcfg, n, k_steps)
        limit = getattr(self, "max_fork_bytes", None)
        if n > 2 ** 31 - 1 or (limit is not None and need > limit):
            raise ValueError(f"{n} branch environments need {need} bytes of device memory"
                             + (f" (max_fork_bytes = {limit})" if limit is not None else " and more than 2^31 - 1 environments"))

    def _sequences(self, actions):
        """``actions`` [B, K(, A)] or [E, B, K(, A)] -> int32 [E, B, K, A]."""
        E, A = self.num_envs, self._hcfg.num_agents
        a = np.asarray(actions)
        if not np.issubdtype(a.dtype, np.integer):
            raise ValueError("action sequences must be integer ids")
        if A == 1 and a.ndim in (2, 3):
            a = a[..., None]
        elif A == 1 and a.ndim == 4 and a.shape[-1] == 1:
            pass
        elif A > 1 and a.ndim in (3, 4) and a.shape[-1] == A:
            pass
        else:
            raise ValueError(f"action sequences must have shape [B, K{', A' if A > 1 else ''}] or [E, B, K{', A' if A > 1 else ''}]; got {a.shape}")
        if a.ndim == 3:
            a = np.broadcast_to(a, (E, *a.shape))
        if a.shape[0] != E or a.shape[1] < 1 or a.shape[2] < 1:
            raise ValueError(f"action sequences for {E} environments needed (with at least one branch and one step); got {np.shape(actions)}")
        return a.astype(np.int32)

    def score_sequences(self, actions, gamma: float = 1.0, return_details: bool = False):
        """Step B candidate action sequences of K steps from the CURRENT state of every environment with the true simulator and
        return their discounted returns f64 [E, B] ([E, B, A] for several agents): fork -> ``hwy_rollout_device`` ->
        ``hwy_score_device`` on one stream.  ``actions``: ids [B, K] (the same candidates everywhere) or [E, B, K], with a
        trailing agent axis for several agents; validated like ``step`` (KeyError / IndexError).  An episode that ends within a
        sequence is absorbing: its terminal reward counts, nothing after it.  This environment is left exactly as it was.
        ``return_details``: also a dict with ``reward`` [E, B, K(, A)], ``terminated`` / ``truncated`` [E, B, K],
        ``best_branch`` [E(, A)] and, single agent, ``q`` [E, n_ids] (the best return per first action, -inf where no
        sequence starts with it) and ``best_action`` [E]."""
        self._lookahead_scope("score_sequences")
        if not np.isfinite(gamma):
            raise ValueError("gamma must be finite")
        a = self._sequences(actions)
        E, B, K, A = a.shape
        self._lookahead_fits(E * B, K)
        child = self.fork(B)
        out = child._engine.score_rollout(np.ascontiguousarray(a.transpose(2, 0, 1, 3)).reshape(K, E * B, A), B, gamma)
        returns = out["returns"] if A > 1 else out["returns"][:, :, 0]
        if not return_details:
            return returns
        reward = out["reward"].reshape(K, E, B, A).transpose(1, 2, 0, 3)
        details = {"reward": reward if A > 1 else reward[..., 0],
                   "terminated": out["terminated"].reshape(K, E, B).transpose(1, 2, 0),
                   "truncated": out["truncated"].reshape(K, E, B).transpose(1, 2, 0),
                   "best_branch": out["best_branch"] if A > 1 else out["best_branch"][:, 0]}
        if A == 1:
            details["q"], details["best_action"] = out["q"], out["best_action"]
        return returns, details

    def lookahead_table(self, depth: int, horizon: int | None = None) -> np.ndarray:
        """The exhaustive depth-``depth`` candidates of ``plan_lookahead``: int32 [n_ids ** depth, horizon]; branch b's first
        ``depth`` actions are the base-n_ids digits of b, most significant first, steps depth .. horizon - 1 are IDLE."""
        if self._hcfg.num_agents > 1:
            raise NotImplementedError("plan_lookahead plans for a single agent (joint-action trees are outside the MI355X hot-path "
                                      "scope): score_sequences serves several agents")
        if self._hcfg.ego_control != _abi.EGO_META:
            raise NotImplementedError("plan_lookahead needs a DiscreteMetaAction ego (a DiscreteAction table has no IDLE) and is "
                                      "outside the MI355X hot-path scope with DiscreteAction: score_sequences serves it")
        depth = int(depth)
        horizon = depth if horizon is None else int(horizon)
        if depth < 1:
            raise ValueError("depth must be >= 1")
        if horizon < depth:
            raise ValueError(f"horizon ({horizon}) must be >= depth ({depth})")
        n_ids = _abi.num_actions(self._hcfg)
        if n_ids ** depth > 2 ** 31 - 1:
            raise ValueError(f"{n_ids} ** {depth} branches per environment do not fit")
        key = (depth, horizon, n_ids)
        cache = self.__dict__.setdefault("_lookahead_tables", {})
        if key not in cache:
            b = np.arange(n_ids ** depth)
            table = np.full((b.size, horizon), 1, np.int32)  # IDLE: id 1 of every meta-action table (action.py:204-222)
            for j in range(depth):
                table[:, j] = (b // n_ids ** (depth - 1 - j)) % n_ids
            cache[key] = table
        return cache[key]

    def plan_lookahead(self, depth: int, horizon: int | None = None, gamma: float = 1.0, return_q: bool = False, masked: bool = False):
        """The best first meta-action int32 [E] of an exhaustive search of depth ``depth`` with the TRUE simulator (every traffic
        vehicle reacts, changes lanes, crashes), where ``plan_finite_mdp`` plans on the reference's constant-speed TTC grid:
        all ``n_ids ** depth`` sequences, padded with IDLE to ``horizon`` steps (default: ``depth``), are stepped from the
        current state and the first action of the best discounted return is returned (the first maximum, numpy's argmax);
        with ``return_q`` also the best return per first action f64 [E, n_ids].  Single agent with a meta-action ego;
        ValueError when the ``E * n_ids ** depth`` branch environments do not fit.
        ``masked``: only the FIRST action is masked -- ``q[e, i] = -inf`` where action ``i`` is not available now
        (``get_available_actions``) and the action returned is the first maximum over the rest.  Masks at the deeper states of
        the open-loop sequences are not applied."""
        self._lookahead_scope("plan_lookahead")
        table = self.lookahead_table(depth, horizon)
        self._lookahead_fits(self.num_envs * table.shape[0], table.shape[1])
        _, details = self.score_sequences(table, gamma=gamma, return_details=True)
        action, q = details["best_action"], details["q"]
        if masked:
            q = np.where(self.get_available_actions(), q, -np.inf)
            action = q.argmax(axis=1).astype(np.int32)
        return (action, q) if return_q else action

    # ---- plan_opd: the budgeted tree search of scripts/highway_planning.ipynb (OPD, csrc/hwy_opd.h) ------------------------------
    def _opd_setup(self, budget, gamma, masked=False):
        """(params, tree, work) of ``plan_opd``: the checks, then the two cached child environments (E * nodes environments that
        hold every node's state, E * n_ids that step the children), auto-reset off."""
        self._lookahead_scope("plan_opd")
        if self._hcfg.num_agents > 1:
            raise NotImplementedError("plan_opd plans for a single agent (joint-action trees are outside the MI355X hot-path scope)")
        if masked and self._hcfg.ego_control != _abi.EGO_META:
            raise NotImplementedError("plan_opd(masked=True) needs a DiscreteMetaAction ego")
        params = _abi.opd_params(self._hcfg, budget, gamma, masked)
        E = self.num_envs
        need, limit = _abi.opd_bytes(self._hcfg, E, params), getattr(self, "max_fork_bytes", None)
        if E * params.nodes > 2 ** 31 - 1 or (limit is not None and need > limit):
            raise ValueError(f"plan_opd: {E} trees of {params.nodes} nodes need {need} bytes of device memory"
                             + (f" (max_fork_bytes = {limit})" if limit is not None else " and more than 2^31 - 1 environments"))
        tree = self._fork_child(("opd", E * params.nodes), E * params.nodes, "plan_opd")
        work = self._fork_child(("opd", E * params.n_ids), E * params.n_ids, "plan_opd")
        return params, tree, work

    def plan_opd(self, budget: int = 50, gamma: float = 0.7, return_details: bool = False, masked: bool = False):
        """The first action int32 [E] of an optimistic plan (OPD, Hren & Munos 2008) of every environment: what the reference's
        ``DeterministicPlannerAgent`` does with ``copy.deepcopy(env)`` + ``env.step`` in scripts/highway_planning.ipynb
        (``budget = 50``, ``gamma = 0.7``), restated in DESIGN.md -- not bit parity with ``rl_agents``.  One tree of at most
        ``1 + budget`` nodes per environment, grown where the optimistic bound is highest by ``budget // n_ids`` expansions with
        the TRUE simulator, entirely on the device (``hwy_opd_plan``).  Single agent, either action type, ``normalize_reward``
        on.  This environment is left exactly as it was.  ``return_details``: also a dict with ``value`` / ``upper`` f64 [E] (the
        bounds on the best discounted return from here), ``sequence`` int32 [E, X] (the plan, padded with -1) and ``expanded``
        int32 [E] (expansions made: fewer than X where the tree was solved).  ``masked``: a node's unavailable actions
        (``get_available_actions`` of its state, by the mask kernel on the work engine) get no child, as in the reference's node
        expansion; the budget still buys ``budget // n_ids`` expansions, and no action of the returned sequence is unavailable
        in the state it is applied to."""
        params, tree, work = self._opd_setup(budget, gamma, masked)
        out = self._engine.opd_plan(tree._engine, work._engine, params)
        if not return_details:
            return out["action"]
        return out["action"], {k: out[k] for k in ("value", "upper", "sequence", "expanded")}

    # ---- score_sequences_continuous / plan_cem: the planning seam for continuous control (csrc/hwy_cem.h) -------------------------
    def _continuous_sequences(self, actions, size: int) -> np.ndarray:
        """``actions`` [B, K(, A), size] or [E, B, K(, A), size] -> float32 [E, B, K, A, size] (a float64 array is ROUNDED first)."""
        E, A = self.num_envs, self._hcfg.num_agents
        a = np.asarray(actions, np.float32)
        want = f"[B, K{', A' if A > 1 else ''}, {size}] or [E, B, K{', A' if A > 1 else ''}, {size}]"
        if a.ndim < 3 or a.shape[-1] != size:
            raise ValueError(f"continuous action sequences must have shape {want}; got {a.shape}")
        if A == 1 and a.ndim in (3, 4):
            a = a[..., None, :]
        elif not (a.ndim in (4, 5) and a.shape[-2] == A):
            raise ValueError(f"continuous action sequences must have shape {want}; got {a.shape}")
        if a.ndim == 4:
            a = np.broadcast_to(a, (E, *a.shape))
        if a.ndim != 5 or a.shape[0] != E or a.shape[1] < 1 or a.shape[2] < 1:
            raise ValueError(f"continuous action sequences for {E} environments needed (with at least one branch and one step); got {np.shape(actions)}")
        return a

    def score_sequences_continuous(self, actions, gamma: float = 1.0, return_details: bool = False):
        """``score_sequences`` for the reference's ``ContinuousAction``: B candidate sequences of K float actions (throttle,
        steering in [-1, 1]; float32 ``[B, K, size]`` or ``[E, B, K, size]``, an agent axis before ``size`` for several agents,
        validated like ``step_continuous``) are stepped from the CURRENT state with the true simulator -- fork ->
        ``hwy_rollout_continuous_device`` -> ``hwy_score_device`` -- and their discounted returns f64 [E, B] ([E, B, A]) come
        back.  An episode that ends within a sequence is absorbing.  This environment is left exactly as it was.
        ``return_details``: also ``reward`` [E, B, K(, A)], ``terminated`` / ``truncated`` [E, B, K] and ``best_branch`` [E(, A)]
        (a float sequence has no first action id: no ``q``, no ``best_action``).  NotImplementedError outside the highway ids
        and on a ``DiscreteMetaAction`` ego."""
        params = self.continuous_params()
        self._lookahead_scope("score_sequences_continuous")
        if not np.isfinite(gamma):
            raise ValueError("gamma must be finite")
        a = self._continuous_sequences(actions, params.size)
        E, B, K, A, size = a.shape
        self._lookahead_fits(E * B, K)
        child = self.fork(B)
        out = child._engine.score_rollout_continuous(params, np.ascontiguousarray(a.transpose(2, 0, 1, 3, 4)).reshape(K, E * B, A, size), B, gamma)
        returns = out["returns"] if A > 1 else out["returns"][:, :, 0]
        if not return_details:
            return returns
        reward = out["reward"].reshape(K, E, B, A).transpose(1, 2, 0, 3)
        return returns, {"reward": reward if A > 1 else reward[..., 0],
                         "terminated": out["terminated"].reshape(K, E, B).transpose(1, 2, 0),
                         "truncated": out["truncated"].reshape(K, E, B).transpose(1, 2, 0),
                         "best_branch": out["best_branch"] if A > 1 else out["best_branch"][:, 0]}

    def _cem_setup(self, population, elites, iterations, horizon, gamma, init_std, min_std, alpha, seed, debug=False):
        """(continuous params, cem params, work) of ``plan_cem``: the checks, then the cached child of E * population environments."""
        cp = self.continuous_params()
        self._lookahead_scope("plan_cem")
        if self._hcfg.num_agents > 1:
            raise NotImplementedError("plan_cem plans for a single agent (joint searches are outside the MI355X hot-path scope): "
                                      "score_sequences_continuous serves several agents")
        if seed is None:  # successive decisions draw different noise; an explicit seed is used as given
            seed = self._cem_default_seed()
        cem = _abi.cem_params(population, elites, iterations, horizon, gamma, init_std, min_std, alpha, seed)
        E = self.num_envs
        n = E * cem.population
        need, limit = _abi.cem_bytes(self._hcfg, E, cem, cp.size, debug), getattr(self, "max_fork_bytes", None)
        if n > 2 ** 31 - 1 or (limit is not None and need > limit):
            raise ValueError(f"{n} branch environments need {need} bytes of device memory"
                             + (f" (max_fork_bytes = {limit})" if limit is not None else " and more than 2^31 - 1 environments"))
        return cp, cem, self._fork_child(("cem", n), n, "plan_cem")

    def _cem_default_seed(self) -> int:
        """The Philox key of a ``plan_cem(seed=None)``: hashed from the seed of ``reset()``, the env's step count and the number of
        default-seed decisions since ``reset()`` -- the last because the device-pointer fronts (``HighwayVectorEnv`` with
        ``output="torch"``) step the engine without passing through ``step`` here, so the step count alone would stand still."""
        key = (int(getattr(self, "_same_step_entropy", 0)) & (2 ** 64 - 1), int(self.steps), self._cem_decisions)
        self._cem_decisions += 1
        return int(np.random.SeedSequence(key).generate_state(1, np.uint64)[0])

    def _cem_init_mean(self, init_mean, K: int, size: int):
        if init_mean is None:
            return None
        m = np.asarray(init_mean, np.float64)
        if m.shape == (K, size):
            m = np.broadcast_to(m, (self.num_envs, K, size))
        if m.shape != (self.num_envs, K, size):
            raise ValueError(f"init_mean must have shape ({K}, {size}) or ({self.num_envs}, {K}, {size}); got {m.shape}")
        if not np.isfinite(m).all():
            raise ValueError("init_mean must be finite")
        return np.ascontiguousarray(m)

    def plan_cem(self, population: int = 64, elites: int = 8, iterations: int = 3, horizon: int = 8, gamma: float = 0.9,
                 init_std: float = 0.5, min_std: float = 0.05, alpha: float = 1.0, seed: int | None = None, init_mean=None,
                 return_details: bool = False, debug: bool = False):
        """Sampling MPC for a continuous ego: the first action float32 [E, size] of a cross-entropy-method search of every
        environment, entirely on the device (``hwy_cem_plan``; DESIGN.md "CEM on the device" states the rules).  Per iteration
        ``population`` sequences of ``horizon`` actions are drawn around the current mean (branch 0 IS the mean), stepped from the
        current state with the TRUE simulator, and mean and std are refitted to the ``elites`` best; the best sequence seen over
        all iterations gives the action.  ``seed=None``: derived from the seed of ``reset()``, the env's step count and the number
        of default-seed decisions since ``reset()``, so that successive decisions do not reuse noise on any front end; an explicit ``seed`` is used as given (same seed, same plan).  ``init_mean``:
        f64 [K, size] or [E, K, size] -- shift the returned ``mean`` by one step and pass it back to warm-start.  This environment
        is left exactly as it was.  ``return_details``: also a dict with ``best_return`` f64 [E], ``best_sequence`` f32
        [E, K, size], ``mean`` / ``std`` f64 [E, K, size]; with ``debug`` also ``noise`` f64 / ``samples`` f32 [I, E, B, K, size] and
        ``elites`` int32 [I, E, M] (every iteration's elite branches, ascending).
        Single agent, ``DiscreteAction`` config, highway ids; NotImplementedError otherwise."""
        cp, cem, work = self._cem_setup(population, elites, iterations, horizon, gamma, init_std, min_std, alpha, seed, debug)
        out = self._engine.cem_plan(work._engine, cp, cem, self._cem_init_mean(init_mean, cem.horizon, cp.size), debug=debug)
        if not return_details:
            return out["action"]
        keys = ("best_return", "best_sequence", "mean", "std") + (("noise", "samples", "elites") if debug else ())
        return out["action"], {k: out[k] for k in keys}

    def close(self) -> None:
        for child in self.__dict__.pop("_forks", {}).values():
            child.close()
        if self._engine is not None:
            self._engine.close()
            self._engine = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchedHighwayEnvFast(BatchedHighwayEnv):
    """E parallel ``highway-fast-v0`` environments (HighwayEnvFast, highway_env.py:154-182)."""
    FAST = True


class BatchedMergeEnv(BatchedHighwayEnv):
    """E parallel ``merge-v0`` environments (MergeEnv, highway_env/envs/merge_env.py:15-190): a two-lane highway,
    an access ramp (``SineLane``) converging onto a forbidden acceleration lane that ends in an ``Obstacle``."""
    SCENARIO = "merge"
    GENERIC = False

    @classmethod
    def default_config(cls) -> dict:
        return _merge.merge_generic_default_config() if cls.GENERIC else _merge.merge_default_config()

    def _spawn_reference(self, generators) -> dict:
        return _merge.spawn_reference_stream(self._hcfg, self.config, self.GENERIC, generators)

    def _device_spawn_args(self) -> dict:
        return {}  # _make_vehicles has no spacing / density / lane parameters (merge_env.py:162-187, 320-363)

    def rewards(self, env_index: int = 0, action=None) -> dict:
        """MergeEnv._rewards (merge_env.py:62-77) of one env, from the device state.  ``action``: the ego's last
        meta-action (the reference evaluates ``action in [0, 2]``); None -> lane_change_reward False."""
        st = self._engine.get_state()
        c = self._hcfg
        e = env_index
        v = st["speed"][e, 0]
        r0, r1 = self.config["reward_speed_range"]
        tab = _merge.table_from_config(c)
        present = (st["flags"][e] & (_abi.F_ABSENT | _abi.F_OBSTACLE)) == 0
        on_merge = present & (st["lane"][e] == c.merge_lane) if c.merge_lane >= 0 else np.zeros_like(present)
        ts, sp = st["target_speed"][e][on_merge], st["speed"][e][on_merge]
        return {"collision_reward": float(bool(st["flags"][e, 0] & _abi.F_CRASHED)),
                "right_lane_reward": float(tab["id"][st["lane"][e, 0]]) / 1,
                "high_speed_reward": float(0 + (v - r0) * (1 - 0) / (r1 - r0)),
                "lane_change_reward": bool(action is not None and np.ndim(action) == 0 and int(action) in (0, 2)),
                "merging_speed_reward": float(np.sum((ts - sp) / ts))}


class BatchedMergeGenericEnv(BatchedMergeEnv):
    """E parallel ``merge-generic-v0`` environments (MergeGenericEnv, merge_env.py:193-371): configurable lane
    count, traffic count and section lengths; ``controlled_vehicles`` > 1 gives BASELINE config 5's multi-agent
    variant (see highwayenv_amd/merge.py)."""
    SCENARIO = "merge-generic"
    GENERIC = True


class _ConnectedLaneNeighboursMixin:
    """ConnectedLaneNeighboursMixin (envs/common/abstract.py:26-37): ``neighbour_vehicles_connected_lanes`` on --
    Road.neighbour_vehicles also searches the lane segments connected to the queried one (road.py:508-529)."""

    @classmethod
    def default_config(cls) -> dict:
        cfg = super().default_config()
        cfg["neighbour_vehicles_connected_lanes"] = True
        return cfg


class BatchedConnectedLaneMergeEnv(_ConnectedLaneNeighboursMixin, BatchedMergeEnv):
    """E parallel ``merge-v1`` environments (ConnectedLaneMergeEnv, merge_env.py:189)."""


class BatchedConnectedLaneMergeGenericEnv(_ConnectedLaneNeighboursMixin, BatchedMergeGenericEnv):
    """E parallel ``merge-generic-v1`` environments (ConnectedLaneMergeGenericEnv, merge_env.py:378)."""


class BatchedIntersectionEnv(BatchedHighwayEnv):
    """E parallel ``intersection-v0`` environments (IntersectionEnv, highway_env/envs/intersection_env.py): a 4-way
    junction of straight and circular lanes, planned routes, ``RegulatedRoad`` priorities, traffic that is cleared and
    spawned while the episode runs, 3 longitudinal meta-actions, Kinematics ``15 x 7`` absolute observation.

    ``spawn_mode="reference"``: traffic management replays the reference's numpy stream on the host
    (``highwayenv_amd/intersection.py``; ``reset(seed=s)`` and every later spawn are the reference's);
    ``spawn_mode="device"``: the step kernel clears / spawns / resets on Philox draws (no host round trip).
    ``config["max_vehicles"]`` (default 32) is the number of vehicle slots per environment."""
    SCENARIO = "intersection"

    @classmethod
    def default_config(cls) -> dict:
        return _ix.intersection_default_config()

    def _define_spaces(self):
        self.config["host_traffic"] = self.spawn_mode == "reference"
        super()._define_spaces()
        A = self._hcfg.num_agents
        if _gym is not None:
            one = _gym.spaces.Discrete(3)
            # MultiAgentAction.space / MultiAgentObservation.space: a Tuple with one entry per agent (action.py:336-340,
            # observation.py:727-731); the observations come stacked as ONE [A, 15, 7] array instead of a tuple of A
            self.single_action_space = one if A == 1 else _gym.spaces.Tuple([one] * A)
        else:
            self.single_action_space = _Discrete(3) if A == 1 else _Tuple([_Discrete(3)] * A)
        self.action_space = self.single_action_space

    def _device_spawn_args(self) -> dict:
        return {}

    def _ego_slots(self, st) -> np.ndarray:  # the ego's slot moves when the vehicle list is re-compacted
        return np.argmax((st["flags"] & _abi.F_CONTROLLED) != 0, axis=1)

    def reset(self, *, seed=None, options: dict | None = None):
        if self.spawn_mode != "reference":
            return super().reset(seed=seed, options=options)
        if options and "config" in options:
            self.configure(options["config"])
        self._define_spaces()
        eng = self._ensure_engine()
        E = self.num_envs
        seeds = [None] * E if seed is None else ([int(seed) + e for e in range(E)] if np.ndim(seed) == 0 else list(seed))
        for e, s in enumerate(seeds):
            if s is not None or self._np_randoms[e] is None:
                self._np_randoms[e] = np.random.Generator(np.random.PCG64(np.random.SeedSequence(s)))
        eng.set_autoreset(False)
        st = _ix.reset_reference_stream(eng, self._hcfg, self.config, self._np_randoms)
        obs = eng.observe()
        self.time[:] = 0
        self.steps = 0
        rows, ego = np.arange(E), self._ego_slots(st)
        info = {"speed": st["speed"][rows, ego].copy(), "crashed": (st["flags"][rows, ego] & _abi.F_CRASHED) != 0, "action": None}
        return self._shape_obs(obs), info

    def step(self, action):
        obs, reward, term, trunc, info = super().step(action)
        # IntersectionEnv._reward: the mean of the agents' rewards, summed left to right (:62-66); _info adds the per-agent
        # rewards and "crashed or arrived" flags (:114-122) -- what MultiAgentWrapper hands out as reward / terminated
        agents_rewards, agents = self._agents_step
        A = self._hcfg.num_agents
        if A > 1:
            total = np.zeros(self.num_envs)
            for a in range(A):
                total = total + agents_rewards[:, a]
            reward = total / A
        info["agents_rewards"] = agents_rewards
        info["agents_terminated"] = agents["crashed"] | agents["arrived"]
        if self.spawn_mode == "reference":  # IntersectionEnv.step: _clear_vehicles, _spawn_vehicle (:136-140)
            _ix.clear_and_spawn_reference_stream(self._engine, self._hcfg, self.config, self._np_randoms)
        return obs, reward, term, trunc, info

    def rewards(self, env_index: int = 0) -> dict:
        """IntersectionEnv._rewards (intersection_env.py:68-77): the agents' _agent_rewards (:96-105) averaged, of one env,
        from the device state."""
        st = self._engine.get_state()
        e = env_index
        tab = _ix.table_from_config(self._hcfg)
        r0, r1 = self.config["reward_speed_range"]
        per_agent = []
        for i in np.nonzero(st["flags"][e] & _abi.F_CONTROLLED)[0][:self._hcfg.num_agents]:
            lane = int(st["lane"][e, i])
            s, lat = _ix.lane_local(tab, lane, (st["x"][e, i], st["y"][e, i]))
            scaled = 0 + (st["speed"][e, i] - r0) * (1 - 0) / (r1 - r0)
            on_road = abs(lat) <= tab["width"][lane] / 2 and -5.0 <= s < tab["length"][lane] + 5.0
            per_agent.append({"collision_reward": float(bool(st["flags"][e, i] & _abi.F_CRASHED)),
                              "high_speed_reward": float(np.clip(scaled, 0, 1)),
                              "arrived_reward": float(bool(tab["exit_lane"][lane]) and s >= 25),
                              "on_road_reward": float(on_road)})
        return {name: sum(r[name] for r in per_agent) / len(per_agent) for name in per_agent[0]}


class BatchedMultiAgentIntersectionEnv(BatchedIntersectionEnv):
    """E parallel ``intersection-multi-agent-v0`` environments (MultiAgentIntersectionEnv, intersection_env.py:348-399):
    ``controlled_vehicles`` (default 2, at most 4) MDP vehicles, agent k entering from road ``o{k % 4}``; actions [E, A],
    observations [E, A, 15, 7], ``reward`` the mean of ``info["agents_rewards"]`` [E, A], ``info["agents_terminated"]``."""

    @classmethod
    def default_config(cls) -> dict:
        cfg = _ix.intersection_default_config()
        cfg["action"] = {"type": "MultiAgentAction", "action_config": cfg["action"]}
        cfg["observation"] = {"type": "MultiAgentObservation", "observation_config": cfg["observation"]}
        cfg["controlled_vehicles"] = 2
        return cfg


# with gymnasium installed the single-environment drop-ins ARE gymnasium.Env's (gym.make / wrappers / checkers accept them)
_GYM_BASES = (_gym.Env,) if _gym is not None else ()


class _SingleEnvMixin:
    """E == 1 with the reference's unbatched signature."""

    def __init__(self, config: dict | None = None, render_mode=None, device: int = 0):
        super().__init__(config, num_envs=1, device=device, render_mode=render_mode)
        self.reset()  # AbstractEnv.__init__ resets (abstract.py:89)

    @property
    def np_random(self):
        """gymnasium.Env.np_random: ONE Generator (wrappers and check_env call .integers / .bit_generator on it)."""
        if self._np_randoms[0] is None:
            self._np_randoms[0] = np.random.Generator(np.random.PCG64(np.random.SeedSequence(None)))
        return self._np_randoms[0]

    @np_random.setter
    def np_random(self, value):
        self._np_randoms = [value]

    def reset(self, *, seed=None, options=None):
        obs, info = super().reset(seed=seed, options=options)
        return obs[0], {"speed": float(info["speed"][0]), "crashed": bool(info["crashed"][0]),
                        "action": self.single_action_space.sample(), "rewards": self.rewards(0)}

    def step(self, action):
        obs, reward, term, trunc, info = super().step(np.asarray([action]).reshape(1, -1))
        return (obs[0], float(reward[0]), bool(term[0]), bool(trunc[0]),
                {"speed": float(info["speed"][0]), "crashed": bool(info["crashed"][0]), "action": action,
                 "rewards": self.rewards(0)})

    def step_continuous(self, action):
        """``step`` with a ``ContinuousAction`` array of shape (size,) -- (A, size) under ``MultiAgentAction`` -- in place of the id."""
        a = np.asarray(action, np.float32)
        obs, reward, term, trunc, info = super().step_continuous(a.reshape(1, self._hcfg.num_agents, -1))
        return (obs[0], float(reward[0]), bool(term[0]), bool(trunc[0]),
                {"speed": float(info["speed"][0]), "crashed": bool(info["crashed"][0]), "action": a, "rewards": self.rewards(0)})

    def plan_cem(self, *args, **kwargs):
        """``BatchedHighwayEnv.plan_cem`` of the one environment: the action float32 (size,) -- what ``step_continuous`` takes -- and,
        with ``return_details``, the details without their environment axis (``noise`` / ``samples``: [I, B, K, size], ``elites``: [I, M])."""
        out = super().plan_cem(*args, **kwargs)
        if not isinstance(out, tuple):
            return out[0]
        return out[0][0], {k: (v[:, 0] if k in ("noise", "samples", "elites") else v[0]) for k, v in out[1].items()}

    def ttc_observation(self, horizon: float = 10.0):
        """``TimeToCollisionObservation(env, horizon).observe()``: float32 (3, 3, T); under ``MultiAgentAction`` a tuple with one such
        array per controlled vehicle (MultiAgentObservation.observe, observation.py:603-604)."""
        obs = super().ttc_observation(horizon)[0]
        return obs if self._hcfg.num_agents == 1 else tuple(obs)

    def lidar_observation(self, cells: int = 16, maximum_range: float = 60.0, normalize: bool = True):
        """``LidarObservation(env, cells, maximum_range, normalize).observe()``: float32 (cells, 2); under ``MultiAgentAction`` a
        tuple with one such array per controlled vehicle, as ``step`` returns its observations."""
        obs = super().lidar_observation(cells, maximum_range, normalize)[0]
        return obs if self._hcfg.num_agents == 1 else tuple(obs)

    def to_finite_mdp(self):
        """``AbstractEnv.to_finite_mdp()`` (abstract.py:452-453): horizon 10 s, time step ``1 / policy_frequency``."""
        return super().to_finite_mdp(0)

    def get_available_actions(self):
        """``AbstractEnv.get_available_actions()`` (abstract.py:357): the list of available action ids in the reference's order
        -- IDLE, then LANE_LEFT, LANE_RIGHT, FASTER, SLOWER where available (action.py:262-298) -- or, under
        ``MultiAgentAction``, the ``itertools.product`` of the agents' lists (action.py:327-333)."""
        mask = super().get_available_actions()[0].reshape(self._hcfg.num_agents, -1)
        order = {3: (1, 0, 2), 5: (1, 0, 2, 3, 4)}[mask.shape[1]]   # ids of IDLE, LANE_LEFT, LANE_RIGHT, FASTER, SLOWER
        if mask.shape[1] == 3 and (self._hcfg.scenario == _abi.SCENARIO_INTERSECTION or self._hcfg.action_set == _abi.ACTIONS_SET_LONGI):
            order = (1, 2, 0)                                       # ids of IDLE, FASTER, SLOWER
        lists = [[i for i in order if row[i]] for row in mask]
        if self.config["action"]["type"] == "MultiAgentAction":
            return itertools.product(*lists)
        return lists[0]

    @property
    def vehicle(self) -> VehicleView:
        return self.road().vehicles[self._hcfg.agent_index[0]]

    @property
    def controlled_vehicles(self):
        vs = self.road().vehicles
        return [vs[self._hcfg.agent_index[a]] for a in range(self._hcfg.num_agents)]


class HighwayEnv(_SingleEnvMixin, BatchedHighwayEnv, *_GYM_BASES):
    """Drop-in for ``highway_env.envs.highway_env.HighwayEnv`` (``highway-v0``)."""


class HighwayEnvFast(_SingleEnvMixin, BatchedHighwayEnvFast, *_GYM_BASES):
    """Drop-in for ``highway_env.envs.highway_env.HighwayEnvFast`` (``highway-fast-v0``)."""


class _SingleMergeMixin(_SingleEnvMixin):
    def step(self, action):
        obs, reward, term, trunc, info = BatchedHighwayEnv.step(self, np.asarray([action]).reshape(1, -1))
        return (obs[0], float(reward[0]), bool(term[0]), bool(trunc[0]),
                {"speed": float(info["speed"][0]), "crashed": bool(info["crashed"][0]), "action": action,
                 "rewards": self.rewards(0, action)})


class _SingleIntersectionMixin(_SingleEnvMixin):
    def step(self, action):
        obs, reward, term, trunc, info = super().step(action)
        batched = self._agents_step
        info["agents_rewards"] = tuple(float(r) for r in batched[0][0])
        info["agents_terminated"] = tuple(bool(c or a) for c, a in zip(batched[1]["crashed"][0], batched[1]["arrived"][0]))
        return obs, reward, term, trunc, info

    @property
    def vehicle(self) -> VehicleView:
        return self.controlled_vehicles[0]

    @property
    def controlled_vehicles(self):
        st = self._engine.get_state()
        return [VehicleView(st, 0, int(i)) for i in np.nonzero(st["flags"][0] & _abi.F_CONTROLLED)[0]]


class IntersectionEnv(_SingleIntersectionMixin, BatchedIntersectionEnv, *_GYM_BASES):
    """Drop-in for ``highway_env.envs.intersection_env.IntersectionEnv`` (``intersection-v0``)."""


class MultiAgentIntersectionEnv(_SingleIntersectionMixin, BatchedMultiAgentIntersectionEnv, *_GYM_BASES):
    """Drop-in for ``highway_env.envs.intersection_env.MultiAgentIntersectionEnv`` (``intersection-multi-agent-v0``): ``step``
    takes a tuple of A meta-actions and returns the A observations stacked in one [A, 15, 7] array."""


class BatchedConnectedLaneMultiAgentIntersectionEnv(_ConnectedLaneNeighboursMixin, BatchedMultiAgentIntersectionEnv):
    """E parallel ConnectedLaneMultiAgentIntersectionEnv (intersection_env.py:405-408)."""


class ConnectedLaneMultiAgentIntersectionEnv(_SingleIntersectionMixin, BatchedConnectedLaneMultiAgentIntersectionEnv, *_GYM_BASES):
    """Drop-in for ``highway_env.envs.intersection_env.ConnectedLaneMultiAgentIntersectionEnv``."""


class _MultiAgentWrapperMixin:
    """``MultiAgentWrapper`` (envs/common/abstract.py:468-477), which the reference registers on top of the
    ``intersection-multi-agent-v1`` / ``-v2`` ids: ``reward`` and ``terminated`` become the per-agent tuples of the info dict."""

    def step(self, action):
        obs, _, _, truncated, info = super().step(action)
        return obs, info["agents_rewards"], info["agents_terminated"], truncated, info


class MultiAgentIntersectionEnvV1(_MultiAgentWrapperMixin, MultiAgentIntersectionEnv):
    """Drop-in for ``gym.make("intersection-multi-agent-v1")``: MultiAgentIntersectionEnv under MultiAgentWrapper."""


class MultiAgentIntersectionEnvV2(_MultiAgentWrapperMixin, ConnectedLaneMultiAgentIntersectionEnv):
    """Drop-in for ``gym.make("intersection-multi-agent-v2")``: ConnectedLaneMultiAgentIntersectionEnv under MultiAgentWrapper."""


class _BatchedMultiAgentWrapperMixin:
    def step(self, action):
        obs, _, _, truncated, info = super().step(action)
        return obs, info["agents_rewards"], info["agents_terminated"], truncated, info


class BatchedMultiAgentIntersectionEnvV1(_BatchedMultiAgentWrapperMixin, BatchedMultiAgentIntersectionEnv):
    """E parallel ``intersection-multi-agent-v1``: ``reward`` [E, A] and ``terminated`` [E, A] per agent (the auto-reset of the
    engine still follows the ENVIRONMENT's terminated | truncated)."""


class BatchedMultiAgentIntersectionEnvV2(_BatchedMultiAgentWrapperMixin, BatchedConnectedLaneMultiAgentIntersectionEnv):
    """E parallel ``intersection-multi-agent-v2``."""


class BatchedConnectedLaneIntersectionEnv(_ConnectedLaneNeighboursMixin, BatchedIntersectionEnv):
    """E parallel ``intersection-v2`` environments (ConnectedLaneIntersectionEnv, intersection_env.py:423)."""


class ConnectedLaneIntersectionEnv(_SingleIntersectionMixin, BatchedConnectedLaneIntersectionEnv, *_GYM_BASES):
    """Drop-in for ``highway_env.envs.intersection_env.ConnectedLaneIntersectionEnv`` (``intersection-v2``)."""


class MergeEnv(_SingleMergeMixin, BatchedMergeEnv, *_GYM_BASES):
    """Drop-in for ``highway_env.envs.merge_env.MergeEnv`` (``merge-v0``)."""


class MergeGenericEnv(_SingleMergeMixin, BatchedMergeGenericEnv, *_GYM_BASES):
    """Drop-in for ``highway_env.envs.merge_env.MergeGenericEnv`` (``merge-generic-v0``)."""


class ConnectedLaneMergeEnv(_SingleMergeMixin, BatchedConnectedLaneMergeEnv, *_GYM_BASES):
    """Drop-in for ``highway_env.envs.merge_env.ConnectedLaneMergeEnv`` (``merge-v1``)."""


class ConnectedLaneMergeGenericEnv(_SingleMergeMixin, BatchedConnectedLaneMergeGenericEnv, *_GYM_BASES):
    """Drop-in for ``highway_env.envs.merge_env.ConnectedLaneMergeGenericEnv`` (``merge-generic-v1``)."""


# The ids `highway_env/__init__.py:30-190` registers for this path (gym.make(id) -> the entry-point class): single
# environment and batched class (the -v1 / -v2 multi-agent intersection ids are the reference's classes under its
# MultiAgentWrapper: the drop-ins fold the wrapper in).  Ids of scenarios outside the path (parking, racetrack, roundabout,
# ...) and the continuous-action intersection id raise KeyError.
REGISTRY = {
    "highway-v0": (HighwayEnv, BatchedHighwayEnv),
    "highway-fast-v0": (HighwayEnvFast, BatchedHighwayEnvFast),
    "merge-v0": (MergeEnv, BatchedMergeEnv),
    "merge-v1": (ConnectedLaneMergeEnv, BatchedConnectedLaneMergeEnv),
    "merge-generic-v0": (MergeGenericEnv, BatchedMergeGenericEnv),
    "merge-generic-v1": (ConnectedLaneMergeGenericEnv, BatchedConnectedLaneMergeGenericEnv),
    "intersection-v0": (IntersectionEnv, BatchedIntersectionEnv),
    "intersection-v2": (ConnectedLaneIntersectionEnv, BatchedConnectedLaneIntersectionEnv),
    "intersection-multi-agent-v0": (MultiAgentIntersectionEnv, BatchedMultiAgentIntersectionEnv),
    "intersection-multi-agent-v1": (MultiAgentIntersectionEnvV1, BatchedMultiAgentIntersectionEnvV1),
    "intersection-multi-agent-v2": (MultiAgentIntersectionEnvV2, BatchedMultiAgentIntersectionEnvV2),
}


GYM_NAMESPACE = "highwayenv_amd"


def register_envs(namespace: str | None = GYM_NAMESPACE) -> list:
    """Register the single-environment drop-ins of REGISTRY with gymnasium, like ``highway_env/__init__.py:22-187`` does for
    the reference at import time: ``gym.make("highwayenv_amd/highway-fast-v0", config={...})``.  The ids live in their own
    namespace so that this package and ``highway_env`` can be installed side by side; ``namespace=None`` registers the
    reference's bare ids (for a box without the reference).  Idempotent; returns the ids it registered; does nothing
    (returns []) when gymnasium is not importable.  Importing ``highwayenv_amd`` calls it."""
    if _gym is None:
        return []
    from gymnasium.envs.registration import register, registry
    done = []
    for env_id, (single, _batched) in REGISTRY.items():
        full = f"{namespace}/{env_id}" if namespace else env_id
        if full in registry:
            continue
        register(id=full, entry_point=f"{__name__}:{single.__name__}")
        done.append(full)
    return done


def batched_class(env_id: str):
    """The ``Batched*Env`` class of an id of REGISTRY (accepts the "highwayenv_amd/" namespace prefix too)."""
    return REGISTRY[env_id.split("/", 1)[-1]][1]


def make(env_id: str, config: dict = None, **kwargs):
    """``gym.make(env_id, config=config)`` for the ids of REGISTRY: the drop-in single environment."""
    return REGISTRY[env_id][0](config, **kwargs)


def make_vec(env_id: str, num_envs: int, config: dict = None, **kwargs):
    """``num_envs`` environments of ``env_id`` stepped by one kernel launch (gymnasium "next-step" auto-reset)."""
    return REGISTRY[env_id][1](config, num_envs=num_envs, **kwargs)


def _copy_config(cfg):
    return copy.deepcopy(cfg)
