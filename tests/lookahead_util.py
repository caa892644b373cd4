"""Shared helpers of the lookahead tests (environment fork, scoring of action sequences, plan_lookahead): the fixtures of
tests/golden/lookahead, the backends (``emu`` = tests/emu/emu.py on the CPU, ``hip`` = the engine on the MI355X), the
environment classes on either backend, and the numpy restatement of the return recurrence every output is held to bit for bit."""
from __future__ import annotations

import os

import numpy as np

from highwayenv_amd import _abi, envs
from tests import backends
from tests.backends import BACKENDS, make_engine  # noqa: F401  (re-exported)
from tests.ttc_util import TtcGolden

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lookahead")
TREE = ["la_fast", "la_trunc", "la_v0", "la_linear"]   # single agent, meta-actions: the 25 depth-2 sequences padded to K = 4
EXPLICIT = ["la_ma2", "la_direct"]                     # explicit sequences
FIXTURES = TREE + EXPLICIT
REWARD_ATOL = 1e-9   # tests/golden_util.py's tolerance for rewards


class LookaheadGolden(TtcGolden):
    """A fixture of tests/golden/lookahead: make_golden_lookahead.py's record."""

    def __init__(self, name: str, data: dict | None = None):
        if data is None:
            with np.load(os.path.join(DIR, name + ".npz")) as z:
                data = {k: z[k] for k in z.files}
        super().__init__(name, data)
        self.sequences = np.asarray(data["sequences"], np.int32)   # [B, K, A]
        self.B, self.K = self.sequences.shape[:2]
        self.gamma = float(data["gamma"])

    def branch_state(self) -> dict:
        return self.state("init", time=self.z["branch_time"])

    def load(self, eng, index=None):
        eng.set_state(self.branch_state())
        if eng.cfg.traffic_model == _abi.TRAFFIC_LINEAR:
            eng.set_behavior(self.z["init_behavior"])
        if eng.cfg.ego_control == _abi.EGO_DIRECT:
            agents = [eng.cfg.agent_index[a] for a in range(eng.cfg.num_agents)]
            eng.set_controls(np.ascontiguousarray(self.z["init_act_accel"][:, agents]),
                             np.ascontiguousarray(self.z["init_act_steering"][:, agents]))


def env_class(backend: str, fast: bool = True):
    """BatchedHighwayEnv(Fast) on the backend."""
    return backends.env_class(backend, envs.BatchedHighwayEnvFast if fast else envs.BatchedHighwayEnv)


def with_envs(cfg: _abi.HwyConfig, num_envs: int) -> _abi.HwyConfig:
    out = _abi.HwyConfig.from_buffer_copy(bytes(cfg))
    out.num_envs = num_envs
    return out


def branch_actions(sequences: np.ndarray, E: int) -> np.ndarray:
    """[B, K, A] -> the rollout's action planes [K, E * B, A] (environment e * B + b is branch b of group e)."""
    B, K, A = sequences.shape
    return np.ascontiguousarray(np.broadcast_to(sequences.transpose(1, 0, 2)[:, None], (K, E, B, A)).reshape(K, E * B, A))


def restate_returns(reward, terminated, truncated, gamma: float) -> np.ndarray:
    """The recurrence of include/hwy_engine.h (hwy_score_device) in numpy f64: reward [K, n, A], flags [K, n] -> g [n, A].
    Product and sum are separate operations, as in the kernel."""
    K, n, A = reward.shape
    g, alive, d = np.zeros((n, A)), np.ones(n, bool), np.float64(1.0)
    for k in range(K):
        t = d * reward[k]
        g = np.where(alive[:, None], g + t, g)
        alive = alive & ~(terminated[k].astype(bool) | truncated[k].astype(bool))
        d = d * np.float64(gamma)
    return g


def restate_scores(reward, terminated, truncated, gamma: float, branches: int, first_action=None, n_ids: int = 5) -> dict:
    """Everything hwy_score_device writes, from the per-step outputs: returns [E, B, A], best_branch [E, A] and, with
    ``first_action`` [E * B] (single agent), q [E, n_ids] and best_action [E] -- numpy's max / argmax (first maximum)."""
    K, n, A = reward.shape
    E = n // branches
    ret = restate_returns(reward, terminated, truncated, gamma).reshape(E, branches, A)
    out = {"returns": ret, "best_branch": np.argmax(ret, axis=1).astype(np.int32)}
    if first_action is not None:
        first = np.asarray(first_action).reshape(E, branches)
        q = np.full((E, n_ids), -np.inf)
        for e in range(E):
            for b in range(branches):
                if 0 <= first[e, b] < n_ids:
                    q[e, first[e, b]] = max(q[e, first[e, b]], ret[e, b, 0])
        out["q"], out["best_action"] = q, np.argmax(q, axis=1).astype(np.int32)
    return out


def assert_bits(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == np.float64:
        a, b = a.view(np.uint64), b.view(np.uint64)
    np.testing.assert_array_equal(a, b, err_msg=what)


def assert_states_equal(a: dict, b: dict, what=""):
    for k in _abi.STATE_F64 + _abi.STATE_I32 + ["time"]:
        assert_bits(a[k], b[k], f"{what}: {k}")


def repeat_state(st: dict, index) -> dict:
    return {k: np.ascontiguousarray(st[k][index]) for k in _abi.STATE_F64 + _abi.STATE_I32 + ["time"]}


def highway_config(n: int, fast: bool = True, **over) -> dict:
    """highway(-fast)-v0 with n vehicles in all, twice the default density: lane changes and collisions within a few steps."""
    d = _abi.highway_fast_default_config() if fast else _abi.highway_default_config()
    d.update({"vehicles_count": n - int(over.get("controlled_vehicles", 1)), "vehicles_density": 2.0, **over})
    return d
