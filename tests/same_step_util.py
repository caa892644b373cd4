"""Shared helpers of the SameStep tests (tests/test_same_step_device.py, _vector.py, _mutations.py): the configurations, one engine
class per backend with ``step_same_step`` (the emulation's: tests/emu/emu_same_step.py; the product's: ``HipSameStepEngine`` below,
``Engine.step_same_step_device`` on torch tensors), the comparison of ONE same-step call against TWO next-step calls, and the
comparison of the episodes the two modes describe over many calls.

Episodes end within a handful of calls: ``duration`` 3, twice the default density and an ego that keeps FASTER (full throttle under
``DiscreteAction``); the merge scenarios, which never truncate, end when the ego passes a finish line moved close to its spawn.  The
seeds and the call at which each comparison is made (``ENTRIES``) were picked on the CPU emulation, where the guards below are
checked again in every run: a comparison that saw no episode end fails.
"""
from __future__ import annotations

import numpy as np

from highwayenv_amd import _abi
from tests.emu.emu_same_step import SENTINEL_U8, new_planes

LINEAR = "highway_env.vehicle.behavior.LinearVehicle"
SPAWN = {"ego_spacing": 2.0, "vehicles_density": 2.0}
BASE_SEED = 4242


def _hwy(fast: bool, **over) -> dict:
    d = _abi.highway_fast_default_config() if fast else _abi.highway_default_config()
    d.update({"duration": 3, "vehicles_density": 2.0, "ego_spacing": 2.0, **over})
    return d


def _merge(generic: bool, **over) -> dict:
    from highwayenv_amd import merge
    d = merge.merge_generic_default_config() if generic else merge.merge_default_config()
    d.update(over)
    return d


# name -> (config dict, make_config keywords, E, finish line of a merge scenario or None)
CONFIGS = {
    "fast": (_hwy(True), {"fast": True}, 8, None),
    "v0_2agents": (_hwy(False, vehicles_count=20, controlled_vehicles=2,
                        action={"type": "MultiAgentAction", "action_config": {"type": "DiscreteMetaAction"}},
                        observation={"type": "MultiAgentObservation", "observation_config": {"type": "Kinematics"}}), {}, 4, None),
    "linear": (_hwy(True, other_vehicles_type=LINEAR), {"fast": True}, 4, None),
    "direct": (_hwy(True, action={"type": "DiscreteAction", "steering_range": [-0.1, 0.1]}), {"fast": True}, 4, None),
    "grid": (_hwy(True, observation={"type": "OccupancyGrid"}), {"fast": True}, 4, None),
    "lidar16": (_hwy(True, observation={"type": "LidarObservation", "cells": 16}), {"fast": True}, 4, None),
    "merge": (_merge(False), {"scenario": "merge"}, 4, 100.0),
    "merge_generic_4agents": (_merge(True, lanes_count=3, vehicles_count=12, controlled_vehicles=4,
                                     action={"type": "MultiAgentAction", "action_config": {"type": "DiscreteMetaAction"}},
                                     observation={"type": "MultiAgentObservation", "observation_config": {"type": "Kinematics"}}),
                              {"scenario": "merge-generic"}, 4, 100.0),
    "n65": (_hwy(False, vehicles_count=64), {}, 2, None),
    "n129": (_hwy(False, vehicles_count=128), {}, 2, None),
}
#: the configurations whose episodes end both ways (the merge scenarios never truncate: merge_env.py:81-82)
BOTH_KINDS = tuple(k for k in CONFIGS if not k.startswith("merge"))
# name -> [(reset seed, plain next-step calls before the compared call, the ego's action, stagger)]: no episode ends in the call before
# the compared one (every `done` is 0 at its entry, as always under SameStep), at least one ends in it, and over a configuration's
# entries at least one ends by `terminated` and -- BOTH_KINDS -- one by `truncated` alone.  stagger = k: after warm-up call k the first
# half of the environments is reset again (on both engines), so that the halves are one call apart -- the merge scenarios' egos all
# drive the same 30 m per call and would otherwise all cross the line in the same call, leaving no environment that did not end.
# Picked on the CPU emulation; one_call_against_two checks the conditions again in every run.
ENTRIES = {
    "fast": [(2, 1, "faster", None), (5, 2, "slower", None)],
    "v0_2agents": [(0, 0, "faster", None), (0, 2, "faster", None)],
    "linear": [(0, 0, "faster", None), (0, 2, "faster", None)],
    "direct": [(3, 0, "faster", None), (3, 2, "faster", None)],
    "grid": [(0, 0, "faster", None), (0, 2, "faster", None)],
    "lidar16": [(0, 0, "faster", None), (0, 2, "faster", None)],
    "merge": [(0, 2, "faster", 0)],
    "merge_generic_4agents": [(0, 2, "faster", 0)],
    "n65": [(0, 0, "faster", None), (0, 2, "faster", None)],
    "n129": [(0, 0, "faster", None), (0, 2, "faster", None)],
}


def config(name: str) -> _abi.HwyConfig:
    d, kw, E, finish = CONFIGS[name]
    c = _abi.make_config(d, E, **kw)
    if finish is not None:  # the ego spawns at x = 30 m with 30 m/s: past the line within three policy steps
        c.merge_end_x = finish
    return c


def faster(cfg: _abi.HwyConfig) -> int:
    """The id that keeps the ego accelerating: FASTER, or full throttle with the middle steering entry under DiscreteAction."""
    if cfg.ego_control == _abi.EGO_DIRECT:
        return (cfg.n_accel - 1) * cfg.n_steer + cfg.n_steer // 2
    return {_abi.ACTIONS_SET_ALL: 3}.get(cfg.action_set, 2)


def slower(cfg: _abi.HwyConfig) -> int:
    """SLOWER (the five-action table), or the lowest throttle with the middle steering entry under DiscreteAction."""
    return cfg.n_steer // 2 if cfg.ego_control == _abi.EGO_DIRECT else 4


def has_masks(cfg: _abi.HwyConfig) -> bool:
    return cfg.ego_control == _abi.EGO_META


def make_engine(backend: str, cfg: _abi.HwyConfig):
    if backend == "emu":
        from tests.emu.emu_same_step import SameStepEmuEngine
        return SameStepEmuEngine(cfg)
    return HipSameStepEngine(cfg)


def _hip_base():
    from highwayenv_amd.engine import Engine
    return Engine


class HipSameStepEngine:
    """The product's Engine with the emulation's ``step_same_step``: device planes are torch tensors, pre-filled with the sentinels."""

    def __init__(self, cfg):
        self._eng = _hip_base()(cfg)

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def step_same_step(self, actions, masks: bool = False, without=()) -> dict:
        import torch
        eng = self._eng
        dev = {k: torch.from_numpy(v).cuda() for k, v in new_planes(eng.cfg, masks).items()}
        acts = torch.from_numpy(np.ascontiguousarray(np.asarray(actions, np.int32).reshape(eng.E, eng.A))).cuda()
        torch.cuda.synchronize()
        ptr = {k: 0 if k in without else v.data_ptr() for k, v in dev.items()}
        eng.step_same_step_device(acts.data_ptr(), ptr["obs"], ptr["reward"], ptr["terminated"], ptr["truncated"], ptr["speed"], ptr["crashed"],
                                  ptr["final_obs"], ptr["final_speed"], ptr["final_crashed"], ptr["final_mask"], ptr.get("action_mask", 0),
                                  ptr.get("final_action_mask", 0))
        eng.sync()
        return {k: v.cpu().numpy() for k, v in dev.items()}


def reset_alike(eng, seed: int) -> None:
    eng.reset(seeds=reset_seeds(eng.cfg, seed), **SPAWN)
    eng.set_autoreset(True, base_seed=BASE_SEED + seed, **SPAWN)


def full_state(eng) -> dict:
    """Everything an engine keeps: the state planes, `time`, the Linear family's parameters, a direct-control ego's stored controls
    and, where the engine shows them (the emulation), the episode counters and the `done` marks."""
    st = {k: np.array(v) for k, v in eng.get_state().items()}
    if eng.cfg.traffic_model == _abi.TRAFFIC_LINEAR:
        st["behavior"] = np.array(eng.get_behavior())
    if eng.cfg.ego_control == _abi.EGO_DIRECT:
        st["ctl_accel"], st["ctl_steer"] = (np.array(a) for a in eng.get_controls())
    if hasattr(eng, "episode"):
        st["episode"], st["done"] = np.array(eng.episode), np.array(eng.done)
    return st


def bits(a: np.ndarray) -> np.ndarray:
    """An array as unsigned integers of its item size: equality of bit patterns, NaN sentinels included."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _eq(got, want, what):
    np.testing.assert_array_equal(bits(np.asarray(got)), bits(np.asarray(want).astype(np.asarray(got).dtype)), err_msg=what)


def reset_seeds(cfg, seed: int) -> np.ndarray:
    return np.uint64(1000 * seed) + np.arange(cfg.num_envs, dtype=np.uint64)


def one_call_against_two(backend: str, name: str, seed: int, warmup: int, action: str = "faster", stagger=None, make_y=None) -> tuple:
    """Engines X and Y reset alike and stepped alike through `warmup` next-step calls; then X: step(a), snapshot, step(anything) --
    the second call re-spawns what ended in the first -- against Y: ONE step_same_step(a) with the final planes pre-filled by
    sentinels.  Returns (episodes that ended by `terminated`, by `truncated` alone).  `make_y`: another factory for Y (a mutant)."""
    cfg = config(name)
    X, Y = make_engine(backend, cfg), (make_y or (lambda c: make_engine(backend, c)))(cfg)
    try:
        E, A, masks = cfg.num_envs, cfg.num_agents, has_masks(cfg)
        a = np.full((E, A), {"faster": faster, "slower": slower}[action](cfg), np.int32)
        prev = np.zeros(E, bool)
        for eng in (X, Y):
            reset_alike(eng, seed)
        for t in range(warmup):
            out = X.step(a)
            Y.step(a)
            prev = out[2] | out[3]
            if stagger == t:
                for eng in (X, Y):
                    eng.reset(seeds=reset_seeds(cfg, seed), mask=(np.arange(E) < E // 2).astype(np.uint8), **SPAWN)
                prev[:E // 2] = False
        assert not prev.any(), f"{name}: an episode ended in the call before the compared one: `done` would not be 0 at entry"
        first = X.step(a)
        snap, snap_mask = full_state(X), (X.action_mask() if masks else None)
        second = X.step(np.zeros((E, A), np.int32))  # ("anything": the re-spawned rows ignore it)
        after, after_mask = full_state(X), (X.action_mask() if masks else None)
        y = Y.step_same_step(a, masks=masks)
        y_state = full_state(Y)
        ended = first[2] | first[3]
        what = f"{name} seed {seed} call {warmup}"
        assert ended.any(), f"{what}: no episode ended in the compared call"
        _eq(y["final_mask"], ended.astype(np.uint8), f"{what}: final_mask")
        _eq(y["reward"], first[1], f"{what}: reward is the ending step's")
        _eq(y["terminated"], first[2].astype(np.uint8), f"{what}: terminated")
        _eq(y["truncated"], first[3].astype(np.uint8), f"{what}: truncated")
        sent = new_planes(cfg, masks)
        for rows, src, src_state, label in ((ended, second, after, "ended"), (~ended, first, snap, "others")):
            _eq(y["obs"][rows], src[0][rows], f"{what}: obs of the {label}")
            _eq(y["speed"][rows], src[4]["speed"][rows], f"{what}: info speed of the {label}")
            _eq(y["crashed"][rows], src[4]["crashed"][rows].astype(np.uint8), f"{what}: info crashed of the {label}")
            assert set(y_state) == set(src_state)
            for f in src_state:
                _eq(y_state[f][rows], src_state[f][rows], f"{what}: state {f} of the {label}")
        _eq(y["final_obs"][ended], first[0][ended], f"{what}: final_obs")
        _eq(y["final_speed"][ended], first[4]["speed"][ended], f"{what}: final info speed")
        _eq(y["final_crashed"][ended], first[4]["crashed"][ended].astype(np.uint8), f"{what}: final info crashed")
        for k in ("final_obs", "final_speed", "final_crashed"):
            _eq(y[k][~ended], sent[k][~ended], f"{what}: {k} rows of environments that did not end still hold the sentinel")
        if masks:
            _eq(y["final_action_mask"], snap_mask.astype(np.uint8), f"{what}: final action mask is the post-step state's")
            _eq(y["action_mask"][ended], after_mask[ended].astype(np.uint8), f"{what}: action mask of the new episodes")
            _eq(y["action_mask"][~ended], snap_mask[~ended].astype(np.uint8), f"{what}: action mask of the others")
        if hasattr(Y, "done"):
            assert not Y.done.any(), f"{what}: an environment is left marked done"
        return int((first[2] & ended).sum()), int((first[3] & ~first[2]).sum())
    finally:
        X.close()
        Y.close()


# ---- the same episodes over many calls ------------------------------------------------------------------------------------------------
def stream_action(cfg, e: int, episode: int, k: int) -> int:
    """The action of step k of episode `episode` of environment e: mostly the id that ends episodes, mixed with the others."""
    h = (e * 7919 + episode * 104729 + k * 1299709) % 11
    return faster(cfg) if h < 7 else h % _abi.num_actions(cfg)


def _actions(cfg, episode, k):
    return np.array([[stream_action(cfg, e, int(episode[e]), int(k[e]))] * cfg.num_agents for e in range(cfg.num_envs)], np.int32)


def episode_streams(backend: str, name: str, seed: int, calls: int, same_step: bool) -> list:
    """Per environment the list of its useful steps over `calls` same-step calls (or as many next-step calls as cover them): each
    (episode, k, terminal-or-plain obs, reward, terminated, truncated, speed, crashed, first obs of the next episode or None, its
    info speed or None)."""
    cfg = config(name)
    eng = make_engine(backend, cfg)
    try:
        E = cfg.num_envs
        reset_alike(eng, seed)
        episode, k = np.zeros(E, int), np.zeros(E, int)
        out = [[] for _ in range(E)]
        if same_step:
            for _ in range(calls):
                y = eng.step_same_step(_actions(cfg, episode, k))
                for e in range(E):
                    end = bool(y["final_mask"][e])
                    obs, speed, crashed = ((y["final_obs"][e], y["final_speed"][e], y["final_crashed"][e]) if end else
                                           (y["obs"][e], y["speed"][e], y["crashed"][e]))
                    out[e].append([int(episode[e]), int(k[e]), obs.copy(), y["reward"][e].copy(), bool(y["terminated"][e]),
                                   bool(y["truncated"][e]), speed.copy(), crashed.astype(bool), y["obs"][e].copy() if end else None,
                                   y["speed"][e].copy() if end else None])
                    episode[e], k[e] = (episode[e] + 1, 0) if end else (episode[e], k[e] + 1)
            return out
        pending = np.zeros(E, bool)
        for _ in range(4 * calls):
            if min(len(o) for o in out) >= calls and not pending.any():
                break
            obs, reward, term, trunc, info = eng.step(_actions(cfg, episode, k))
            for e in range(E):
                if pending[e]:  # the re-spawn row: the first observation of the episode that starts
                    out[e][-1][8], out[e][-1][9] = obs[e].copy(), info["speed"][e].copy()
                    assert not term[e] and not trunc[e] and (reward[e] == 0).all() and not info["crashed"][e].any()
                    pending[e] = False
                    continue
                end = bool(term[e] | trunc[e])
                out[e].append([int(episode[e]), int(k[e]), obs[e].copy(), reward[e].copy(), bool(term[e]), bool(trunc[e]),
                               info["speed"][e].copy(), info["crashed"][e].copy(), None, None])
                pending[e] = end
                episode[e], k[e] = (episode[e] + 1, 0) if end else (episode[e], k[e] + 1)
        return [o[:calls] for o in out]
    finally:
        eng.close()


def assert_same_episodes(backend: str, name: str, seed: int, calls: int) -> tuple:
    """SameStep and NextStep describe the same episodes: every useful step of every environment equal, bit for bit, the terminal
    observation and the first observation of the following episode included.  Returns (terminated, truncated-only) endings seen."""
    same, nxt = episode_streams(backend, name, seed, calls, True), episode_streams(backend, name, seed, calls, False)
    n_term = n_trunc = 0
    for e, (s, n) in enumerate(zip(same, nxt)):
        assert len(s) == len(n) == calls, f"{name}: environment {e}: {len(s)} / {len(n)} useful steps"
        for j, (a, b) in enumerate(zip(s, n)):
            what = f"{name} env {e} useful step {j} (episode {a[0]}, step {a[1]})"
            assert a[:2] == b[:2] and a[4:6] == b[4:6], f"{what}: {a[:2]} {a[4:6]} / {b[:2]} {b[4:6]}"
            for i in (2, 3, 6, 7):
                _eq(a[i], b[i], f"{what}: field {i}")
            assert (a[8] is None) == (b[8] is None), what
            if a[8] is not None:
                _eq(a[8], b[8], f"{what}: first observation of the next episode")
                _eq(a[9], b[9], f"{what}: info speed of the next episode's first state")
            n_term += int(a[4])
            n_trunc += int(a[5] and not a[4])
    return n_term, n_trunc


__all__ = ["CONFIGS", "ENTRIES", "BOTH_KINDS", "SENTINEL_U8", "config", "make_engine", "one_call_against_two", "assert_same_episodes"]
