"""A ``gymnasium.vector.VectorEnv``-shaped front end of the batched environments.

What the reference's users plug into their training loops is a vector env -- ``gym.vector.SyncVectorEnv([...],
autoreset_mode="SameStep")`` in ``/root/reference/tests/envs/test_gym.py:158-165``, ``make_vec_env(..., SubprocVecEnv)`` in
``scripts/sb3_highway_ppo.py:16-18`` -- i.e. E Python processes stepping E copies of ``AbstractEnv.step``.  Here the E
environments are ONE engine (one kernel launch per step), and this class gives them that interface:

* ``num_envs``, ``single_observation_space`` / ``single_action_space`` and the batched ``observation_space`` / ``action_space``;
* ``reset(seed=..., options=...) -> (obs [E, ...], infos)``, ``step(actions) -> (obs, rewards f64 [E], terminations, truncations,
  infos)``, ``step_async`` / ``step_wait``, ``close``;
* a DECLARED autoreset mode (``metadata["autoreset_mode"]``, gymnasium >= 1.0 vocabulary):

  - ``"NextStep"`` (default; gymnasium's default too): an environment that ends at step t returns its terminal observation with
    ``terminated`` / ``truncated`` set; the call of step t + 1 re-spawns it INSTEAD of stepping (its action is ignored) and
    returns the first observation of the new episode with reward 0 and both flags False.  That is exactly what the step kernels
    do on the device (``hwy_set_autoreset``), so this mode costs nothing;
  - ``"SameStep"`` (what the reference's vectorisation test asks for): the step that ends an episode already returns the
    first observation of the next one; the terminal observation and info travel in ``infos["final_obs"]`` / ``infos["final_info"]``
    (object arrays, ``None`` where the episode goes on) with the ``_final_obs`` / ``_final_info`` masks.  One masked device reset
    per step in which some episode ended.  With ``output="torch"`` the whole of it happens on the device in the same call
    (``hwy_step_same_step_device``: step, stash of the terminal rows, re-spawn) and the extras are DENSE tensors and a mask instead
    of object arrays: ``final_obs`` [E, ...] and ``final_info = {"speed", "crashed"(, "action_mask")}`` hold the terminal values in
    the rows where the bool mask ``_final_obs`` (== ``_final_info`` == ``terminated | truncated``) is set and are NOT written in the
    other rows (zeros, or an earlier episode's end: read them under the mask); the episodes are those of ``"NextStep"`` on the
    same seed, bit for bit.  Highway and merge ids; the intersection ids raise ``ValueError`` in this combination;
  - ``"Disabled"``: finished environments keep stepping until the caller resets.

* ``output="torch"``: observations, rewards and flags are ``torch`` tensors that ALIAS the buffers the kernel writes (no host
  round trip), actions may be a device tensor, and everything is ordered on torch's current stream -- a policy network can read
  ``obs`` and write ``actions`` without leaving the GPU ("keeping the policy on-GPU").  Every autoreset
  mode.  ``rollout(actions[K])`` exposes ``hwy_rollout_device`` (K steps per launch, NextStep between them) in this mode.
* ``continuous=True`` (an env configured with ``DiscreteAction``): the reference's ``ContinuousAction`` -- ``single_action_space`` is
  ``Box(-1, 1, (size,), float32)`` and ``step`` / ``step_async`` / ``rollout`` take float actions [E(, A), size] (throttle, steering),
  mapped onto the configured ranges by a kernel of its own (csrc/hwy_act.h) in front of the engine's step; every output and every
  autoreset mode as with ids.  A policy network's float32 device tensor goes to the kernel as it is.  ``plan_cem(...)`` plans such
  actions by the cross-entropy method on the device (csrc/hwy_cem.h); with ``output="torch"`` ``env.step(env.plan_cem())`` never
  leaves the GPU.
* ``ttc_observation=True`` (or ``{"horizon": h}``; highway ids with ``DiscreteMetaAction``): the observation is the reference's
  ``TimeToCollisionObservation`` -- ``single_observation_space`` is ``Box(0, 1, (3, 3, T), float32)`` and ``reset`` / ``step`` /
  ``rollout`` / ``final_obs`` hand out that window, computed by a kernel of its own (csrc/hwy_collision_obs.h) behind the engine's
  step; the env's configured observation type is still computed and not returned.  NumPy output: step, observe, masked reset,
  observe.  ``output="torch"``: the device entry points (``hwy_rollout_ttc_device`` with K = 1; SameStep: the one call
  ``hwy_step_same_step_ttc_device``), no host copy anywhere.  Not together with ``continuous=True`` (the egos differ).
* ``lidar_observation=True`` (or ``{"cells": c, "maximum_range": r, "normalize": n}``; highway AND merge ids, any ego, up to 256
  cells): the observation is the reference's ``LidarObservation`` -- ``single_observation_space`` is ``Box(-high, high, (cells, 2),
  float32)`` and ``reset`` / ``step`` / ``rollout`` / ``final_obs`` hand out that trace, computed by a kernel of its own
  (csrc/hwy_lidar_door.h) behind the engine's step; the env's configured observation type is still computed and not returned.
  NumPy output, every autoreset mode: step, observe, masked reset, observe.  ``output="torch"`` (NextStep, Disabled): the step's
  device call -- ids or, with ``continuous=True``, the continuous door -- then ``hwy_lidar_observe_device`` into the tensor handed
  out, on the same stream; ``rollout``: ``hwy_rollout_lidar_device`` (ids only).  ``ValueError``: on the intersection ids (the
  reference observes there BEFORE it clears and spawns vehicles, a kernel behind the step AFTER: ``env.lidar_observation()`` is
  ``observe()`` called after ``step()``, not the observation ``step()`` returns); with ``output="torch"`` and SameStep; together
  with ``ttc_observation``.

With gymnasium installed the class IS a ``gymnasium.vector.VectorEnv``; without it (this image) the same attributes exist on a
plain object.
"""
from __future__ import annotations

import numpy as np

from . import _abi, envs as _envs

try:  # optional
    import gymnasium as _gym
    _Base = _gym.vector.VectorEnv
except Exception:  # pragma: no cover - gymnasium is absent in the build image
    _gym = None
    _Base = object

AUTORESET_MODES = ("NextStep", "SameStep", "Disabled")


class _Batched:
    """Batched view of a single-environment space (stand-in for gymnasium.vector.utils.batch_space without gymnasium)."""

    def __init__(self, single, n):
        self.single, self.n = single, n
        self.shape = (n, *getattr(single, "shape", ()))
        self.dtype = getattr(single, "dtype", None)

    def sample(self):
        return np.stack([np.asarray(self.single.sample()) for _ in range(self.n)])

    def contains(self, x):
        return len(x) == self.n and all(self.single.contains(v) for v in x)


class HighwayVectorEnv(_Base):
    """E environments of one scenario behind the vector-env interface (see the module docstring).

    ``env``: a ``Batched*Env`` class or instance, or an id of ``highwayenv_amd.envs.REGISTRY`` ("highway-fast-v0", "merge-v0",
    "intersection-v0", ...)."""

    def __init__(self, env="highway-fast-v0", num_envs: int = 1, config: dict | None = None, autoreset_mode: str = "NextStep",
                 output: str = "numpy", device: int = 0, spawn_mode: str = "device", stream=None, action_masks: bool = False,
                 continuous: bool = False, ttc_observation=False, lidar_observation=False, **kwargs):
        mode = getattr(autoreset_mode, "value", autoreset_mode)  # gymnasium.vector.AutoresetMode or its string
        mode = {"next_step": "NextStep", "same_step": "SameStep", "disabled": "Disabled"}.get(str(mode).lower(), str(mode))
        if mode not in AUTORESET_MODES:
            raise ValueError(f"autoreset_mode must be one of {AUTORESET_MODES}")
        if output not in ("numpy", "torch"):
            raise ValueError("output must be 'numpy' or 'torch'")
        self.autoreset_mode = mode
        # output="torch" with SameStep: the engine runs with auto-reset enabled and every step is one hwy_step_same_step_device
        self._device_same_step = output == "torch" and mode == "SameStep"
        scenario = getattr(_envs.batched_class(env) if isinstance(env, str) else env, "SCENARIO", None)
        if self._device_same_step and scenario == "intersection":
            raise ValueError("output='torch' with autoreset_mode='SameStep' is not available for the intersection scenario (its next "
                             "episodes are pre-warmed on the device, keyed to the episode counter); use NextStep, or output='numpy'")
        self.output = output
        # lidar_observation: the observations of reset / step / rollout / final_obs are the reference's LidarObservation traces,
        # float32 [E(, A), cells, 2] (csrc/hwy_lidar_door.h), in place of the env's configured observation type.
        self._lidar_params = None
        if lidar_observation is not False and lidar_observation is not None:  # ({}: the defaults)
            if ttc_observation is not False and ttc_observation is not None:
                raise ValueError("lidar_observation and ttc_observation both replace the observation: not together")
            if scenario == "intersection":
                raise ValueError("lidar_observation is not available for the intersection scenario: the reference's step() observes "
                                 "BEFORE it clears and spawns vehicles, a kernel behind the step sees the list AFTER them, so the trace "
                                 "is observe() called after step(), not the observation step() returns (env.lidar_observation() "
                                 "hands out exactly that)")
            if self._device_same_step:
                raise ValueError("lidar_observation with output='torch' and autoreset_mode='SameStep' is not available (it takes a "
                                 "SameStep sequence of its own on the device); use NextStep, or output='numpy'")
            opts = dict(lidar_observation) if isinstance(lidar_observation, dict) else {}
            unknown = set(opts) - {"cells", "maximum_range", "normalize"}
            if unknown:
                raise ValueError(f"lidar_observation: unknown keys {sorted(unknown)}")
            self._lidar_params = _abi.lidar_door_params(opts.get("cells", 16), opts.get("maximum_range", 60.0), opts.get("normalize", True))
        # action_masks: reset() and step() put info["action_mask"] (gymnasium's convention) into the info dict: bool [E, n_ids]
        # ([E, A, n_ids] for several agents), the mask of the state whose observation is returned (csrc/hwy_mask.h).  With
        # output="torch" it is the device tensor the kernel wrote.  False: nothing more is launched.
        self.action_masks = bool(action_masks)
        if output == "torch":
            import torch  # the device-pointer path: torch owns the output tensors and the stream
            self._torch = torch
            torch.cuda.set_device(device)
            # the engine gets a stream of its own (the handle of torch's default stream is NULL, which hwy_create reads as
            # "create one"); every call orders it after the caller's current stream and the caller's stream after it.
            # ``stream=`` (a torch.cuda.Stream, not the default one): the engine runs ON that stream, and a step() issued while
            # it is the current stream needs no cross-stream ordering at all (two event record / wait pairs less per step).
            if stream is None:  # built under `with torch.cuda.stream(s)`: that stream; under the default stream: a new one
                cur = torch.cuda.current_stream(device)
                stream = cur if cur.cuda_stream else torch.cuda.Stream(device=device)
            self._stream = stream
            stream = self._stream.cuda_stream
            if not stream:
                raise ValueError("stream= must be a real torch.cuda.Stream (the default stream's handle is NULL)")
        elif stream is not None:
            raise ValueError("stream= needs output='torch'")
        if isinstance(env, str):
            env = _envs.batched_class(env)
        engine_autoreset = mode == "NextStep" or self._device_same_step
        if isinstance(env, type):
            env = env(config, num_envs=num_envs, device=device, spawn_mode=spawn_mode, autoreset=engine_autoreset,
                      stream=stream, **kwargs)
        elif config:
            env.configure(config)
        self.env = env
        env.autoreset = engine_autoreset
        self.num_envs = env.num_envs
        self.single_observation_space, self.single_action_space = env.single_observation_space, env.single_action_space
        # continuous: the actions of step / step_async / rollout are the reference's ContinuousAction arrays -- float32 [E(, A), size]
        # in [-1, 1], size 2 (throttle, steering) or 1 -- in place of DiscreteAction ids; the env is configured with a DiscreteAction
        # (same vehicle class, same ranges and axes) and every call goes through the engine's continuous entry points (csrc/hwy_act.h).
        self.continuous = bool(continuous)
        self._cparams = None
        if self.continuous:
            if env._hcfg.ego_control != _abi.EGO_DIRECT:
                raise ValueError("continuous=True needs an env configured with {'type': 'DiscreteAction'} (a plain-Vehicle ego)")
            self._cparams = env.continuous_params()
            self.single_action_space = env.continuous_action_space()  # Box(-1, 1, (size,), float32); several agents: as for Discrete
        # ttc_observation: the observations of reset / step / rollout / final_obs are the reference's TimeToCollisionObservation
        # windows, float32 [E(, A), 3, 3, T] (csrc/hwy_collision_obs.h), in place of the env's configured observation type.
        self._ttc_horizon = None
        if ttc_observation is not False and ttc_observation is not None:  # ({}: the default horizon)
            if self.continuous:
                raise ValueError("ttc_observation needs a DiscreteMetaAction ego and continuous=True a DiscreteAction ego: not together")
            h = ttc_observation.get("horizon", 10.0) if isinstance(ttc_observation, dict) else 10.0
            self._ttc_horizon = float(h)
            self.single_observation_space = env.ttc_observation_space(self._ttc_horizon)  # NotImplementedError outside the scope
            self._ttc_params = env._ttc_obs_params(self._ttc_horizon, need_engine=False)
        if self._lidar_params is not None:
            self._lidar_kw = {"cells": self._lidar_params.cells, "maximum_range": self._lidar_params.maximum_range,
                              "normalize": bool(self._lidar_params.normalize)}
            self.single_observation_space = env.lidar_observation_space(**self._lidar_kw)
        if _gym is not None:
            self.observation_space = _gym.vector.utils.batch_space(self.single_observation_space, self.num_envs)
            self.action_space = _gym.vector.utils.batch_space(self.single_action_space, self.num_envs)
        else:
            self.observation_space = _Batched(self.single_observation_space, self.num_envs)
            self.action_space = _Batched(self.single_action_space, self.num_envs)
        self.metadata = {"autoreset_mode": (getattr(_gym.vector, "AutoresetMode", None)(_snake(mode))
                                            if _gym is not None and hasattr(_gym.vector, "AutoresetMode") else mode),
                         "render_modes": []}
        self.render_mode = None
        self.closed = False
        self._pending = None
        self._needs_reset = np.zeros(self.num_envs, bool)  # SameStep bookkeeping is immediate; NextStep lives in the engine
        self._dev = None

    # ---- reset / step ------------------------------------------------------------------------------------------------------
    def reset(self, *, seed=None, options=None):
        obs, info = self.env.reset(seed=seed, options=options)
        if self._ttc_horizon is not None:
            self._ttc_params = self.env._ttc_obs_params(self._ttc_horizon)
            obs = None if self.output == "torch" else self.env.ttc_observation(self._ttc_horizon)
        if self._lidar_params is not None:
            obs = None if self.output == "torch" else self.env.lidar_observation(**self._lidar_kw)
        self._needs_reset[:] = False
        infos = {"speed": np.asarray(info["speed"], np.float64), "crashed": np.asarray(info["crashed"], bool)}
        if self.output == "torch":
            self._bind_device_buffers()
            t = self._torch
            if self.action_masks:
                self._mask_into(self._dev["action_mask"])
                infos["action_mask"] = self._views["action_mask"]
            if self._ttc_horizon is not None:  # observed on the device into a tensor of its own (the next step overwrites the view)
                first = t.empty_like(self._dev["obs"])
                self._ordered(lambda: self.env._engine.ttc_observe_device(self._ttc_params, first.data_ptr()), first)
                return (first[:, 0] if first.shape[1] == 1 else first), infos
            if self._lidar_params is not None:
                first = t.empty_like(self._dev["obs"])
                self._ordered(lambda: self.env._engine.lidar_observe_device(self._lidar_params, first.data_ptr()), first)
                return (first[:, 0] if first.shape[1] == 1 else first), infos
            return t.from_numpy(np.ascontiguousarray(obs)).to(self._dev["obs"].device), infos
        if self.action_masks:
            infos["action_mask"] = self.env.get_available_actions()
        return obs, infos

    def step_async(self, actions) -> None:
        self._pending = actions

    def step_wait(self):
        actions, self._pending = self._pending, None
        if actions is None:
            raise RuntimeError("step_wait() without step_async()")
        return self.step(actions)

    def step(self, actions):
        if self.output == "torch":
            return self._step_torch(actions)
        obs, reward, term, trunc, info = self.env.step_continuous(actions) if self.continuous else self.env.step(actions)
        infos = {"speed": np.asarray(info["speed"], np.float64), "crashed": np.asarray(info["crashed"], bool)}
        for k in ("agents_rewards", "agents_terminated", "rewards"):
            if k in info:
                infos[k] = info[k]
        done = term | trunc
        if self._ttc_horizon is not None:  # of the state the step left: the terminal window where an episode ended
            obs = self.env.ttc_observation(self._ttc_horizon)
        if self._lidar_params is not None:  # the trace of the state the step left: the terminal one where an episode ended
            obs = self.env.lidar_observation(**self._lidar_kw)
        if self.action_masks:
            infos["action_mask"] = self.env.get_available_actions()
        if self.autoreset_mode == "SameStep" and done.any():
            obs = np.array(obs, copy=True)
            final_obs = np.full(self.num_envs, None, dtype=object)
            final_info = np.full(self.num_envs, None, dtype=object)
            for e in np.nonzero(done)[0]:
                final_obs[e] = obs[e].copy()
                final_info[e] = {"speed": float(infos["speed"][e]), "crashed": bool(infos["crashed"][e])}
                if self.action_masks:  # the ended episode's mask
                    final_info[e]["action_mask"] = infos["action_mask"][e].copy()
            if self._lidar_params is not None:  # the new episodes' traces (the other rows: the same state, the same values)
                self.env.reset_done(done)
                obs = self.env.lidar_observation(**self._lidar_kw)
            elif self._ttc_horizon is None:
                obs[done] = self.env.reset_done(done)
            else:  # the new episodes' windows (the other rows: the same state, the same values)
                self.env.reset_done(done)
                obs = self.env.ttc_observation(self._ttc_horizon)
            if self.action_masks:      # ... and the new episode's, next to its observation
                infos["action_mask"] = self.env.get_available_actions()
            infos.update({"final_obs": final_obs, "_final_obs": done.copy(), "final_info": final_info, "_final_info": done.copy()})
        return obs, np.asarray(reward, np.float64), term, trunc, infos

    # ---- device-resident outputs ------------------------------------------------------------------------------------------------
    def _bind_device_buffers(self):
        t, E, A = self._torch, self.num_envs, self.env._hcfg.num_agents
        dev = t.device("cuda", self.env.device)
        shape = self._obs_shape()
        self._dev = {"obs": t.empty((E, A, *shape), dtype=t.float32, device=dev), "reward": t.empty((E, A), dtype=t.float64, device=dev),
                     "terminated": t.empty(E, dtype=t.uint8, device=dev), "truncated": t.empty(E, dtype=t.uint8, device=dev),
                     "speed": t.empty((E, A), dtype=t.float64, device=dev), "crashed": t.empty((E, A), dtype=t.uint8, device=dev)}
        d = self._dev
        if self.action_masks:
            if self.env._hcfg.ego_control != _abi.EGO_META:
                raise NotImplementedError("action_masks needs a DiscreteMetaAction ego")
            d["action_mask"] = t.empty((E, A, _abi.num_actions(self.env._hcfg)), dtype=t.uint8, device=dev)
        if self._device_same_step:  # the planes of the terminal rows (hwy_step_same_step_device writes the rows of ended episodes)
            d["final_obs"], d["final_speed"] = t.zeros_like(d["obs"]), t.zeros_like(d["speed"])
            d["final_crashed"], d["final_mask"] = t.zeros_like(d["crashed"]), t.zeros(E, dtype=t.uint8, device=dev)
            if self.action_masks:
                d["final_action_mask"] = t.zeros_like(d["action_mask"])
        self._n_actions = E * A * (self._cparams.size if self.continuous else 1)
        self._action_dtype = t.float32 if self.continuous else t.int32
        self._out_ptrs = tuple(d[k].data_ptr() for k in ("obs", "reward", "terminated", "truncated", "speed", "crashed"))
        if self._lidar_params is not None:  # the step's own observation goes to a tensor nobody reads; d["obs"] takes the trace
            d["step_obs"] = t.empty((E, A, *_abi.obs_shape(self.env._hcfg)), dtype=t.float32, device=dev)
            self._out_ptrs = (d["step_obs"].data_ptr(),) + self._out_ptrs[1:]
        # what step() hands out: views of the planes the kernel writes (bool views of the 0 / 1 flag bytes; the intersection's
        # info_crashed carries has_arrived in bit 1, include/hwy_engine.h, so its `crashed` is computed per step)
        plain_crashed = self.env._hcfg.scenario != _abi.SCENARIO_INTERSECTION
        self._views = {"obs": d["obs"][:, 0] if A == 1 else d["obs"], "reward": d["reward"][:, 0],
                       "terminated": d["terminated"].view(t.bool), "truncated": d["truncated"].view(t.bool),
                       "speed": d["speed"][:, 0], "crashed": d["crashed"][:, 0].view(t.bool) if plain_crashed else None}
        if self.action_masks:  # the 0 / 1 bytes the mask kernel writes, as a zero-copy bool view
            self._views["action_mask"] = (d["action_mask"][:, 0] if A == 1 else d["action_mask"]).view(t.bool)
        if self._device_same_step:
            self._final_ptrs = tuple(d[k].data_ptr() if k in d else 0 for k in (
                "final_obs", "final_speed", "final_crashed", "final_mask", "action_mask", "final_action_mask"))
            v = self._views
            v["final_obs"] = d["final_obs"][:, 0] if A == 1 else d["final_obs"]
            v["final_mask"] = d["final_mask"].view(t.bool)
            v["final_info"] = {"speed": d["final_speed"][:, 0], "crashed": d["final_crashed"][:, 0].view(t.bool)}
            if self.action_masks:
                v["final_info"]["action_mask"] = (d["final_action_mask"][:, 0] if A == 1 else d["final_action_mask"]).view(t.bool)

    def _obs_shape(self) -> tuple:
        """Shape of one agent's observation as this front end hands it out."""
        if self._lidar_params is not None:
            return _abi.lidar_door_shape(self._lidar_params)
        return _abi.obs_shape(self.env._hcfg) if self._ttc_horizon is None else _abi.ttc_obs_shape(self._ttc_params)

    def _ordered(self, enqueue, *tensors):
        """``enqueue()`` on the engine's stream, ordered after the caller's current stream and the caller's stream after it."""
        cur = self._torch.cuda.current_stream()
        same = cur.cuda_stream == self._stream.cuda_stream
        if not same:
            self._stream.wait_stream(cur)
        enqueue()
        if not same:
            cur.wait_stream(self._stream)
            for x in tensors:
                x.record_stream(self._stream)

    def _mask_into(self, out):
        """Enqueue the mask kernel into the uint8 device tensor ``out`` on the engine's stream, ordered after the caller's current
        stream and the caller's stream after it (nothing to order when they are the same stream)."""
        cur = self._torch.cuda.current_stream()
        same = cur.cuda_stream == self._stream.cuda_stream
        if not same:
            self._stream.wait_stream(cur)
        self.env._engine.action_mask_device(out.data_ptr())
        if not same:
            cur.wait_stream(self._stream)

    def _device_actions(self, actions, lead=()):
        t, E, A = self._torch, self.num_envs, self.env._hcfg.num_agents
        a = actions if isinstance(actions, t.Tensor) else t.as_tensor(np.asarray(actions))
        if self.continuous:  # float32 [*lead, E(, A), size] (a float64 tensor is rounded to float32, like the numpy path)
            size = self._cparams.size
            a = a.to(device=self._dev["obs"].device, dtype=t.float32)
            if a.dim() == len(lead) + 2 and A > 1:
                a = a.unsqueeze(-2).expand(*lead, E, A, size)
            return a.reshape(*lead, E, A, size).contiguous()
        a = a.to(device=self._dev["obs"].device, dtype=t.int32)
        if a.dim() == len(lead) + 1 and A > 1:
            a = a.unsqueeze(-1).expand(*lead, E, A)
        return a.reshape(*lead, E, A).contiguous()

    def _step_torch(self, actions):
        """One launch on torch's stream; the returned tensors alias the engine's output buffers (valid until the next step).
        Action ids are NOT validated on this path (include/hwy_engine.h: hwy_step_device); ids outside the table act as IDLE.
        The host side of a step is kept to the launch and two stream waits: no elementwise kernel is launched for the outputs
        (the flag planes hold 0 / 1 bytes and are returned as zero-copy bool VIEWS), and an int32 device tensor of the right
        shape goes to the kernel as it is.  ``continuous=True``: the same with a float32 device tensor [E(, A), size] and the
        continuous entry points (the act kernel, then the step launch, on the same stream; a NaN row keeps its stored controls)."""
        t, d = self._torch, self._dev
        if not (isinstance(actions, t.Tensor) and actions.dtype == self._action_dtype and actions.is_cuda and actions.is_contiguous()
                and actions.numel() == self._n_actions):
            actions = self._device_actions(actions)
        cur = t.cuda.current_stream()
        same = cur.cuda_stream == self._stream.cuda_stream
        if not same:
            self._stream.wait_stream(cur)      # the actions (and the consumer of the previous outputs) come first
        if self._ttc_horizon is not None and self._device_same_step:  # step, observe, stash, re-spawn, observe in one call
            self.env._engine.step_same_step_ttc_device(self._ttc_params, actions.data_ptr(), *self._out_ptrs, *self._final_ptrs)
        elif self._ttc_horizon is not None:    # the step launch, then the window of the state it left
            self.env._engine.rollout_ttc_device(self._ttc_params, 1, actions.data_ptr(), *self._out_ptrs)
            if self.action_masks:
                self.env._engine.action_mask_device(d["action_mask"].data_ptr())
        elif self.continuous and self._device_same_step:
            self.env._engine.step_same_step_continuous_device(self._cparams, actions.data_ptr(), *self._out_ptrs, *self._final_ptrs)
        elif self.continuous:
            self.env._engine.step_continuous_device(self._cparams, actions.data_ptr(), *self._out_ptrs)
        elif self._device_same_step:           # step, stash of the terminal rows, re-spawn (and both masks) in one call
            self.env._engine.step_same_step_device(actions.data_ptr(), *self._out_ptrs, *self._final_ptrs)
        else:
            self.env._engine.step_device(actions.data_ptr(), *self._out_ptrs)
            if self.action_masks:              # of the state this step left, behind it on the engine's stream
                self.env._engine.action_mask_device(d["action_mask"].data_ptr())
        if self._lidar_params is not None:     # the trace of the state the step left, behind it on the engine's stream
            self.env._engine.lidar_observe_device(self._lidar_params, d["obs"].data_ptr())
        if not same:
            cur.wait_stream(self._stream)      # whatever the caller enqueues next sees this step's outputs
            actions.record_stream(self._stream)
        v = self._views
        infos = {"speed": v["speed"], "crashed": v["crashed"] if v["crashed"] is not None else (d["crashed"][:, 0] & 1).bool()}
        if self.action_masks:
            infos["action_mask"] = v["action_mask"]
        if self._device_same_step:             # dense tensors under a mask (the numpy path hands out object arrays)
            infos.update({"final_obs": v["final_obs"], "_final_obs": v["final_mask"], "final_info": v["final_info"],
                          "_final_info": v["final_mask"]})
        return v["obs"], v["reward"], v["terminated"], v["truncated"], infos

    def rollout(self, actions):
        """``actions`` [K, E(, A)] -> (obs [K, E, ...], rewards [K, E], terminations [K, E], truncations [K, E]) as device tensors:
        K policy steps in one call of ``hwy_rollout_device`` (one LAUNCH on the one-wavefront kernel), NextStep autoreset between
        the steps.  ``output="torch"`` only."""
        if self._lidar_params is not None and self.continuous:
            raise ValueError("rollout() with lidar_observation and continuous=True is not available (hwy_rollout_lidar_device takes ids)")
        if self.output != "torch":
            raise ValueError("rollout() needs output='torch'")
        t, E, A = self._torch, self.num_envs, self.env._hcfg.num_agents
        K = int(actions.shape[0])
        a = self._device_actions(actions, lead=(K,))
        dev = self._dev["obs"].device
        obs = t.empty((K, E, A, *self._obs_shape()), dtype=t.float32, device=dev)
        rew = t.empty((K, E, A), dtype=t.float64, device=dev)
        term, trunc = t.empty((K, E), dtype=t.uint8, device=dev), t.empty((K, E), dtype=t.uint8, device=dev)
        cur = t.cuda.current_stream()
        self._stream.wait_stream(cur)
        if self._lidar_params is not None:  # K (step, observe) launch pairs enqueued by one call (hwy_rollout_lidar_device)
            self.env._engine.rollout_lidar_device(self._lidar_params, K, a.data_ptr(), obs.data_ptr(), rew.data_ptr(), term.data_ptr(),
                                                  trunc.data_ptr())
        elif self._ttc_horizon is not None:  # K (step, observe) launch pairs enqueued by one call (hwy_rollout_ttc_device)
            self.env._engine.rollout_ttc_device(self._ttc_params, K, a.data_ptr(), obs.data_ptr(), rew.data_ptr(), term.data_ptr(),
                                                trunc.data_ptr())
        elif self.continuous:  # K (act, step) launch pairs enqueued by one call (hwy_rollout_continuous_device)
            self.env._engine.rollout_continuous_device(self._cparams, K, a.data_ptr(), obs.data_ptr(), rew.data_ptr(), term.data_ptr(),
                                                       trunc.data_ptr())
        else:
            self.env._engine.rollout_device(K, a.data_ptr(), obs.data_ptr(), rew.data_ptr(), term.data_ptr(), trunc.data_ptr())
        cur.wait_stream(self._stream)
        for x in (a, obs, rew, term, trunc):
            x.record_stream(self._stream)
        return (obs[:, :, 0] if A == 1 else obs), rew[:, :, 0], term.bool(), trunc.bool()

    def plan(self, gamma: float = 1.0, horizon: float = 10.0):
        """The reference's value-iteration policy on ``to_finite_mdp()`` (envs/common/finite_mdp.py) for every environment, solved
        by the planner kernel: meta-action ids [E] ([E, A] for several agents).  ``output="torch"``: an int32 device tensor that
        aliases the buffer the kernel writes (valid until the next ``plan()``), ordered on the current stream like ``step`` --
        ``env.step(env.plan())`` never leaves the GPU."""
        if self.output != "torch":
            return self.env.plan_finite_mdp(gamma=gamma, horizon=horizon)
        params = self.env._ttc_params(horizon, None, gamma)
        t, A = self._torch, self.env._hcfg.num_agents
        if self._dev is None:
            raise RuntimeError("plan() before reset()")
        if "plan" not in self._dev:
            self._dev["plan"] = t.empty((self.num_envs, A), dtype=t.int32, device=self._dev["obs"].device)
        out = self._dev["plan"]
        cur = t.cuda.current_stream()
        same = cur.cuda_stream == self._stream.cuda_stream
        if not same:
            self._stream.wait_stream(cur)      # the consumer of the previous plan comes first
        self.env._engine.mdp_plan_device(params, out.data_ptr())
        if not same:
            cur.wait_stream(self._stream)
        return out[:, 0] if A == 1 else out

    # ---- simulator-based planning: fork -> rollout -> score on the engine's stream -----------------------------------------------------
    def _lookahead_device(self, a, B, K, gamma):
        """``a``: int32 device tensor [K, E * B, A] of action ids (not validated on this path, like ``step``).  Enqueues the fork
        of the current state, the K-step rollout of the branches and the fold, ordered on the caller's stream like ``plan``;
        returns the dict of device tensors the three wrote (cached per shape: valid until the next call of that shape)."""
        t, env = self._torch, self.env
        E, A = self.num_envs, env._hcfg.num_agents
        if self._dev is None:
            raise RuntimeError("plan_lookahead() / score_sequences() before reset()")
        env._lookahead_fits(E * B, K)
        n, ids, dev = E * B, _abi.num_actions(env._hcfg), self._dev["obs"].device
        key = ("lookahead", B, K)
        if key not in self._dev:
            child = env.fork(B)   # (allocates the branch engine on the engine's stream; forks once more below)
            self._dev[key] = {
                "child": child, "obs": t.empty((K, n, A, *_abi.obs_shape(env._hcfg)), dtype=t.float32, device=dev),
                "reward": t.empty((K, n, A), dtype=t.float64, device=dev), "terminated": t.empty((K, n), dtype=t.uint8, device=dev),
                "truncated": t.empty((K, n), dtype=t.uint8, device=dev), "returns": t.empty((E, B, A), dtype=t.float64, device=dev),
                "best_branch": t.empty((E, A), dtype=t.int32, device=dev),
                "q": t.empty((E, ids), dtype=t.float64, device=dev) if A == 1 else None,
                "best_action": t.empty(E, dtype=t.int32, device=dev) if A == 1 else None}
        d = self._dev[key]
        child = d["child"]._engine
        ptr = lambda x: 0 if x is None else x.data_ptr()  # noqa: E731
        cur = t.cuda.current_stream()
        same = cur.cuda_stream == self._stream.cuda_stream
        if not same:
            self._stream.wait_stream(cur)      # the actions (and the consumer of the previous scores) come first
        child.fork_device(env._engine, B)
        child.rollout_device(K, a.data_ptr(), d["obs"].data_ptr(), d["reward"].data_ptr(), d["terminated"].data_ptr(),
                             d["truncated"].data_ptr())
        child.score_device(K, B, gamma, a.data_ptr() if A == 1 else 0, d["reward"].data_ptr(), d["terminated"].data_ptr(),
                           d["truncated"].data_ptr(), d["returns"].data_ptr(), ptr(d["q"]), ptr(d["best_action"]),
                           d["best_branch"].data_ptr())
        if not same:
            cur.wait_stream(self._stream)
            a.record_stream(self._stream)
        return d

    def score_sequences(self, actions, gamma: float = 1.0, return_details: bool = False):
        """``BatchedHighwayEnv.score_sequences`` for every environment.  ``output="torch"``: ``actions`` may be a device tensor
        ([B, K(, A)] or [E, B, K(, A)]), the returns [E, B(, A)] (and, with ``return_details``, the per-step rewards and flags,
        ``q``, ``best_action``, ``best_branch``) are device tensors ordered on the current stream like ``plan()``; nothing visits
        the host, and action ids are not validated (as in ``step``)."""
        if self.output != "torch":
            return self.env.score_sequences(actions, gamma=gamma, return_details=return_details)
        t, E, A = self._torch, self.num_envs, self.env._hcfg.num_agents
        self.env._lookahead_scope("score_sequences")
        a = actions if isinstance(actions, t.Tensor) else t.as_tensor(np.asarray(actions))
        if A == 1 and a.dim() in (2, 3):
            a = a.unsqueeze(-1)
        if a.dim() == 3:
            a = a.unsqueeze(0).expand(E, *a.shape)
        if a.dim() != 4 or a.shape[0] != E or a.shape[3] != A:
            raise ValueError(f"action sequences must have shape [B, K{', A' if A > 1 else ''}] or [E, B, K{', A' if A > 1 else ''}]")
        B, K = int(a.shape[1]), int(a.shape[2])
        dev = self._dev["obs"].device if self._dev is not None else None
        a = a.to(device=dev, dtype=t.int32).permute(2, 0, 1, 3).reshape(K, E * B, A).contiguous()
        d = self._lookahead_device(a, B, K, float(gamma))
        returns = d["returns"] if A > 1 else d["returns"][:, :, 0]
        if not return_details:
            return returns
        reward = d["reward"].view(K, E, B, A).permute(1, 2, 0, 3)
        details = {"reward": reward if A > 1 else reward[..., 0], "terminated": d["terminated"].view(K, E, B).permute(1, 2, 0).bool(),
                   "truncated": d["truncated"].view(K, E, B).permute(1, 2, 0).bool(),
                   "best_branch": d["best_branch"] if A > 1 else d["best_branch"][:, 0]}
        if A == 1:
            details["q"], details["best_action"] = d["q"], d["best_action"]
        return returns, details

    def plan_lookahead(self, depth: int, horizon: int | None = None, gamma: float = 1.0, return_q: bool = False, masked: bool = False):
        """``BatchedHighwayEnv.plan_lookahead``: the best first meta-action [E] of an exhaustive depth-``depth`` search with the true
        simulator.  ``output="torch"``: an int32 device tensor (valid until the next call of that shape) ordered on the current
        stream -- ``env.step(env.plan_lookahead(2))`` never leaves the GPU; the candidate table is built once on the host and
        uploaded.  ``masked``: ``q`` is -inf where the FIRST action is not available now (the mask kernel's output, on the device)
        and the action is the first maximum over the rest; deeper states of the open-loop sequences are not masked."""
        if self.output != "torch":
            return self.env.plan_lookahead(depth, horizon=horizon, gamma=gamma, return_q=return_q, masked=masked)
        t, E = self._torch, self.num_envs
        self.env._lookahead_scope("plan_lookahead")
        table = self.env.lookahead_table(depth, horizon)
        B, K = table.shape
        if self._dev is None:
            raise RuntimeError("plan_lookahead() before reset()")
        key = ("lookahead_table", B, K)
        if key not in self._dev:   # [K, E * B, 1]: the same candidates in every environment
            planes = np.ascontiguousarray(np.broadcast_to(table.T[:, None, :], (K, E, B)).reshape(K, E * B, 1))
            self._dev[key] = t.from_numpy(planes).to(self._dev["obs"].device)
        d = self._lookahead_device(self._dev[key], B, K, float(gamma))
        if masked:
            if "lookahead_mask" not in self._dev:
                self._dev["lookahead_mask"] = t.empty((E, 1, _abi.num_actions(self.env._hcfg)), dtype=t.uint8, device=self._dev["obs"].device)
            m = self._dev["lookahead_mask"]
            self._mask_into(m)
            q = t.where(m[:, 0].view(t.bool), d["q"], t.full_like(d["q"], float("-inf")))
            action = q.argmax(dim=1).to(t.int32)   # (torch's argmax returns the first maximum on ties, like numpy's)
            return (action, q) if return_q else action
        return (d["best_action"], d["q"]) if return_q else d["best_action"]

    def plan_opd(self, budget: int = 50, gamma: float = 0.7, return_details: bool = False, masked: bool = False):
        """``BatchedHighwayEnv.plan_opd``: the first action [E] of an optimistic plan (OPD) of every environment, grown by
        ``budget // n_ids`` expansions with the true simulator.  ``output="torch"``: an int32 device tensor (and, with
        ``return_details``, device tensors ``value``, ``upper``, ``sequence``, ``expanded``; all valid until the next call of that
        shape), ordered on the current stream like ``plan()`` -- the whole loop is enqueued by one ``hwy_opd_plan_device`` call
        and ``env.step(env.plan_opd())`` never leaves the GPU.  ``masked``: unavailable actions get no child."""
        if self.output != "torch":
            return self.env.plan_opd(budget, gamma, return_details=return_details, masked=masked)
        t, E, env = self._torch, self.num_envs, self.env
        params, tree, work = env._opd_setup(budget, gamma, masked)
        if self._dev is None:
            raise RuntimeError("plan_opd() before reset()")
        X, dev = params.budget // params.n_ids, self._dev["obs"].device
        key = ("opd", X)
        if key not in self._dev:
            self._dev[key] = {"action": t.empty(E, dtype=t.int32, device=dev), "value": t.empty(E, dtype=t.float64, device=dev),
                              "upper": t.empty(E, dtype=t.float64, device=dev), "sequence": t.empty((E, X), dtype=t.int32, device=dev),
                              "expanded": t.empty(E, dtype=t.int32, device=dev)}
        d = self._dev[key]
        cur = t.cuda.current_stream()
        same = cur.cuda_stream == self._stream.cuda_stream
        if not same:
            self._stream.wait_stream(cur)      # the consumer of the previous plan comes first
        env._engine.opd_plan_device(tree._engine, work._engine, params, *(d[k].data_ptr() for k in ("action", "value", "upper", "sequence", "expanded")))
        if not same:
            cur.wait_stream(self._stream)
        if not return_details:
            return d["action"]
        return d["action"], {k: d[k] for k in ("value", "upper", "sequence", "expanded")}

    def plan_cem(self, population: int = 64, elites: int = 8, iterations: int = 3, horizon: int = 8, gamma: float = 0.9,
                 init_std: float = 0.5, min_std: float = 0.05, alpha: float = 1.0, seed: int | None = None, init_mean=None,
                 return_details: bool = False, debug: bool = False):
        """``BatchedHighwayEnv.plan_cem``: the first action float32 [E, size] of a cross-entropy-method search of every environment
        (``continuous=True``).  ``output="torch"``: the device tensor the refit kernel wrote (and, with ``return_details``, device
        tensors ``best_return``, ``best_sequence``, ``mean``, ``std``; all valid until the next call of that shape), ordered on the
        current stream like ``plan()`` -- the whole search is enqueued by one ``hwy_cem_plan_device`` call and
        ``env.step(env.plan_cem())`` never leaves the GPU.  ``init_mean``: a float64 array or device tensor [K, size] or
        [E, K, size]; a device tensor is not validated.  ``debug``: the details also hold ``noise`` f64 / ``samples`` f32
        [I, E, B, K, size] and ``elites`` int32 [I, E, M].  ``seed=None`` draws a new Philox key per decision (the env counts them),
        although this path steps the engine without advancing the env's step count."""
        if not self.continuous:
            raise ValueError("plan_cem needs continuous=True (an env configured with {'type': 'DiscreteAction'})")
        if self.output != "torch":
            return self.env.plan_cem(population, elites, iterations, horizon, gamma, init_std, min_std, alpha, seed, init_mean,
                                     return_details=return_details, debug=debug)
        t, E, env = self._torch, self.num_envs, self.env
        cp, cem, work = env._cem_setup(population, elites, iterations, horizon, gamma, init_std, min_std, alpha, seed, debug)
        if self._dev is None:
            raise RuntimeError("plan_cem() before reset()")
        K, size, dev = cem.horizon, cp.size, self._dev["obs"].device
        key = ("cem", K)
        if key not in self._dev:
            self._dev[key] = {"action": t.empty((E, size), dtype=t.float32, device=dev), "best_return": t.empty(E, dtype=t.float64, device=dev),
                              "mean": t.empty((E, K, size), dtype=t.float64, device=dev), "std": t.empty((E, K, size), dtype=t.float64, device=dev),
                              "best_sequence": t.empty((E, K, size), dtype=t.float32, device=dev)}
        d = self._dev[key]
        dbg = {}
        if debug:  # (allocated per call: a test's door, not the hot path)
            shape = (cem.iterations, E, cem.population, K, size)
            dbg = {"noise": t.empty(shape, dtype=t.float64, device=dev), "samples": t.empty(shape, dtype=t.float32, device=dev),
                   "elites": t.empty((cem.iterations, E, cem.elites), dtype=t.int32, device=dev)}
        im = None
        if init_mean is not None:
            if isinstance(init_mean, t.Tensor):
                im = init_mean.to(device=dev, dtype=t.float64)
                im = (im.unsqueeze(0).expand(E, K, size) if im.dim() == 2 else im).reshape(E, K, size).contiguous()
            else:
                im = t.from_numpy(env._cem_init_mean(init_mean, K, size)).to(dev)
        cur = t.cuda.current_stream()
        same = cur.cuda_stream == self._stream.cuda_stream
        if not same:
            self._stream.wait_stream(cur)      # the consumer of the previous plan (and init_mean) comes first
        env._engine.cem_plan_device(work._engine, cp, cem, d["action"].data_ptr(), 0 if im is None else im.data_ptr(),
                                    *(d[k].data_ptr() for k in ("best_return", "mean", "std", "best_sequence")),
                                    *(dbg[k].data_ptr() for k in ("noise", "samples", "elites") if debug))
        if not same:
            cur.wait_stream(self._stream)
            for x in ([im] if im is not None else []) + list(dbg.values()):
                x.record_stream(self._stream)
        if not return_details:
            return d["action"]
        return d["action"], dict({k: d[k] for k in ("best_return", "best_sequence", "mean", "std")}, **dbg)

    # ---- the rest of the interface ----------------------------------------------------------------------------------------------
    @property
    def stream(self):
        """output='torch': the torch.cuda.Stream the engine launches on (the ``stream=`` argument, or the one created for it).
        A step() issued while it is the CURRENT stream (``with torch.cuda.stream(venv.stream): ...``) needs no cross-stream
        ordering: 44.6 us per step at 4096 x 51 against 68 with an event wait on either side of the launch."""
        return getattr(self, "_stream", None)

    def close(self, **kwargs):
        if not self.closed:
            self.env.close()
            self.closed = True

    def close_extras(self, **kwargs):
        self.close()

    @property
    def unwrapped(self):
        return self

    def call(self, name, *args, **kwargs):
        """gymnasium.vector.VectorEnv.call: the batched environment is ONE object; its answer is returned once per environment."""
        attr = getattr(self.env, name)
        out = attr(*args, **kwargs) if callable(attr) else attr
        return tuple(out for _ in range(self.num_envs))

    def get_attr(self, name):
        return self.call(name)


def _snake(mode: str) -> str:
    return {"NextStep": "NextStep", "SameStep": "SameStep", "Disabled": "Disabled"}[mode]
