"""Shared helpers of the TimeToCollision observation tests: the fixtures of tests/golden/ttc_obs, one engine class per backend with
``ttc_observe`` / ``step_ttc`` / ``rollout_ttc`` / ``step_same_step_ttc`` (the emulation's: tests/emu/emu_ttc_obs.py; the product's:
``HipTtcObsEngine`` below, the device-pointer entry points on torch tensors), and the closed form of the reference's slicing."""
from __future__ import annotations

import os

import numpy as np

from highwayenv_amd import _abi
from tests.backends import BACKENDS  # noqa: F401  (re-exported)
from tests.emu.emu_same_step import new_planes
from tests.ttc_util import TtcGolden

OBS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ttc_obs")
# tests/golden/ttc_obs/make_golden_ttc_obs.py: SCENARIOS
FIXTURES = ["ttcobs_fast", "ttcobs_lanes1", "ttcobs_lanes2", "ttcobs_lanes16", "ttcobs_speeds2", "ttcobs_speeds8", "ttcobs_horizon1",
            "ttcobs_pf5", "ttcobs_t64", "ttcobs_ma2", "ttcobs_edges", "ttcobs_ladder", "ttcobs_crash", "ttcobs_alone"]


class TtcObsGolden(TtcGolden):
    """A fixture of tests/golden/ttc_obs: the states of a run and the reference's ``observe()`` of every controlled vehicle,
    ``obs0`` [E, A, 3, 3, T] at reset and ``obs`` [steps, E, A, 3, 3, T]."""

    def __init__(self, name: str, data: dict | None = None):
        if data is None:
            with np.load(os.path.join(OBS_DIR, name + ".npz")) as z:
                data = {k: z[k] for k in z.files}
        super().__init__(name, data)
        # the reference ran with the TimeToCollision type, which the engine's config rejects: the engine is created with the
        # Kinematics observation and hands the window out through its own entry points
        self.reference_observation = self.config["observation"]
        kinematics = {"type": "Kinematics"}
        self.config["observation"] = ({"type": "MultiAgentObservation", "observation_config": kinematics}
                                      if self.reference_observation["type"] == "MultiAgentObservation" else kinematics)


def window(grid: np.ndarray, lane: int, speed_index: int) -> np.ndarray:
    """The closed form of TimeToCollisionObservation.observe's slicing (observation.py:133-152) for V >= 2: grid [V, L, T] ->
    [3, 3, T], 1.0 where the lane is off the road, the speed index clamped."""
    V, L, T = grid.shape
    out = np.ones((3, 3, T), grid.dtype)
    for a in range(3):
        v = min(max(speed_index + a - 1, 0), V - 1)
        for b in range(3):
            if 0 <= lane + b - 1 < L:
                out[a, b] = grid[v, lane + b - 1]
    return out


def windows(cfg: _abi.HwyConfig, st: dict, grids: np.ndarray) -> np.ndarray:
    """``window`` of every (environment, agent): grids [E, A, V, L, T] and the state they belong to -> [E, A, 3, 3, T]."""
    E, A = grids.shape[:2]
    out = np.empty((E, A, 3, 3, grids.shape[-1]), grids.dtype)
    for e in range(E):
        for a in range(A):
            i = cfg.agent_index[a]
            out[e, a] = window(grids[e, a], int(st["lane"][e, i]), int(st["speed_index"][e, i]))
    return out


def bits(a) -> np.ndarray:
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def make_engine(backend: str, cfg: _abi.HwyConfig):
    if backend == "emu":
        from tests.emu.emu_ttc_obs import TtcObsEmuEngine
        return TtcObsEmuEngine(cfg)
    return HipTtcObsEngine(cfg)


class HipTtcObsEngine:
    """The product's Engine with the emulation's method names: device planes are torch tensors, pre-filled with the sentinels."""

    def __init__(self, cfg):
        from highwayenv_amd.engine import Engine
        self._eng = Engine(cfg)

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def ttc_observe_host(self, params):
        return self._eng.ttc_observe(params)

    def ttc_observe(self, params):
        """The DEVICE-pointer form (tests hold it to ``ttc_observe_host``)."""
        import torch
        eng = self._eng
        obs = torch.full((eng.E, eng.A, *_abi.ttc_obs_shape(params)), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        eng.ttc_observe_device(params, obs.data_ptr())
        eng.sync()
        return obs.cpu().numpy()

    def rollout_ttc(self, params, actions):
        import torch
        eng = self._eng
        acts = torch.from_numpy(np.ascontiguousarray(np.asarray(actions, np.int32).reshape(-1, eng.E, eng.A))).cuda()
        K, E, A = acts.shape[0], eng.E, eng.A
        nan = float("nan")
        obs = torch.full((K, E, A, *_abi.ttc_obs_shape(params)), nan, dtype=torch.float32, device="cuda")
        reward, speed = (torch.full((K, E, A), nan, dtype=torch.float64, device="cuda") for _ in range(2))
        term, trunc = (torch.full((K, E), 0xFF, dtype=torch.uint8, device="cuda") for _ in range(2))
        crashed = torch.full((K, E, A), 0xFF, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        eng.rollout_ttc_device(params, K, *(x.data_ptr() for x in (acts, obs, reward, term, trunc, speed, crashed)))
        eng.sync()
        c = crashed.cpu().numpy()
        return (obs.cpu().numpy(), reward.cpu().numpy(), term.cpu().numpy().astype(bool), trunc.cpu().numpy().astype(bool),
                {"speed": speed.cpu().numpy(), "crashed": (c & 1).astype(bool), "arrived": (c & 2).astype(bool)})

    def step_ttc(self, params, actions):
        out = self.rollout_ttc(params, np.asarray(actions, np.int32).reshape(1, self._eng.E, self._eng.A))
        return tuple(o[0] for o in out[:4]) + ({k: v[0] for k, v in out[4].items()},)

    def step_same_step_ttc(self, params, actions, masks: bool = False, without=()) -> dict:
        import torch
        eng = self._eng
        planes = new_planes(eng.cfg, masks)
        for k in ("obs", "final_obs"):
            planes[k] = np.full((eng.E, eng.A, *_abi.ttc_obs_shape(params)), np.nan, np.float32)
        dev = {k: torch.from_numpy(v).cuda() for k, v in planes.items()}
        acts = torch.from_numpy(np.ascontiguousarray(np.asarray(actions, np.int32).reshape(eng.E, eng.A))).cuda()
        torch.cuda.synchronize()
        ptr = {k: 0 if k in without else v.data_ptr() for k, v in dev.items()}
        eng.step_same_step_ttc_device(params, acts.data_ptr(), ptr["obs"], ptr["reward"], ptr["terminated"], ptr["truncated"], ptr["speed"],
                                      ptr["crashed"], ptr["final_obs"], ptr["final_speed"], ptr["final_crashed"], ptr["final_mask"],
                                      ptr.get("action_mask", 0), ptr.get("final_action_mask", 0))
        eng.sync()
        return {k: v.cpu().numpy() for k, v in dev.items()}
