"""Shared helpers of the CEM tests: the plain-NumPy restatement of csrc/hwy_cem.h (DESIGN.md "CEM on the device"), the fixtures of
tests/golden/cem and the backends (``emu`` = tests/emu/emu_cem.py on the CPU, ``hip`` = the engine on the MI355X)."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

from highwayenv_amd import _abi
from highwayenv_amd.envs import BatchedHighwayEnvFast
from tests.spawn_util import philox4x32_10

CEM_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cem")
BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
F32, F64 = np.float32, np.float64
M32 = 0xFFFFFFFF
TWO_PI, PI = 6.283185307179586, 3.141592653589793
#: absolute tolerance of the engine's normals against the float64 NumPy Box-Muller: 4 x the largest difference measured on the CPU
#: emulation over every draw of these tests, 6.66e-16 (profiles/cem.md); hwy_math.h documents ~2 ulp per function and |z| <= 8.6
NOISE_ATOL = 2.7e-15


# ---- the engines -------------------------------------------------------------------------------------------------------------------
def make_engine(backend: str, cfg):
    if backend == "emu":
        from tests.emu.emu_cem import CemEmuEngine
        return CemEmuEngine(cfg)
    from highwayenv_amd.engine import Engine
    return Engine(cfg)


def env_class(backend: str, base=BatchedHighwayEnvFast):
    if backend != "emu":
        return base
    from tests.emu.emu_cem import CemEmuEngine
    return type("Emu" + base.__name__, (base,), {"_engine_factory": staticmethod(lambda cfg, device, stream: CemEmuEngine(cfg))})


def small_config(size: int = 2, vehicles: int = 5, agents: int = 1, **kw) -> dict:
    """6 vehicles (5 + the ego), a narrow steering range so that episodes last; ``size`` 1: longitudinal only."""
    act = {"type": "DiscreteAction", "steering_range": [-0.05, 0.05], "actions_per_axis": 3}
    if size == 1:
        act["lateral"] = False
    cfg = {"vehicles_count": vehicles, "lanes_count": 3, "duration": 30, "action": act}
    if agents > 1:
        cfg["controlled_vehicles"] = agents
        cfg["action"] = {"type": "MultiAgentAction", "action_config": act}
        cfg["observation"] = {"type": "MultiAgentObservation", "observation_config": {"type": "Kinematics"}}
    cfg.update(kw)
    return cfg


def make_env(backend: str, num_envs: int = 3, seed: int = 11, **kw):
    env = env_class(backend)(small_config(**kw), num_envs=num_envs)
    env.reset(seed=seed)
    return env


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def philox_words(seed: int, e: int, b: int, draw: int) -> tuple:
    """The four words of the sample kernel's Philox block: counter (environment, branch, draw, "HWCM"), key = seed."""
    return tuple(philox4x32_10((e, b, draw, _abi.HWY_CEM_STREAM_TAG), (seed & M32, (seed >> 32) & M32)))


def uniforms(words) -> tuple:
    a, b = (words[0] << 32) | words[1], (words[2] << 32) | words[3]
    return (a >> 11) * (1.0 / 9007199254740992.0), (b >> 11) * (1.0 / 9007199254740992.0)


def box_muller(u0, u1):
    """Two standard normals in float64 NumPy: the cosine one (throttle) and the sine one (steering)."""
    u0, u1 = np.asarray(u0, F64), np.asarray(u1, F64)
    r = np.sqrt(-2.0 * np.log(1.0 - u0))
    a = TWO_PI * u1
    a = np.where(a >= PI, a - TWO_PI, a)
    return r * np.cos(a), r * np.sin(a)


def restate_noise(seed: int, E: int, B: int, K: int, size: int, iterations, envs=None) -> np.ndarray:
    """noise f64 [I, E, B, K, size] of the iterations ``iterations`` (an int: range) for the environment indices ``envs``."""
    its = list(range(iterations)) if np.ndim(iterations) == 0 else list(iterations)
    envs = list(range(E)) if envs is None else list(envs)
    u = np.zeros((len(its), len(envs), B, K, 2))
    for ii, i in enumerate(its):
        for ei, e in enumerate(envs):
            for b in range(1, B):
                for k in range(K):
                    u[ii, ei, b, k] = uniforms(philox_words(seed, e, b, i * _abi.HWY_CEM_MAX_HORIZON + k))
    zc, zs = box_muller(u[..., 0], u[..., 1])
    z = np.stack([zc, zs], axis=-1)[..., :size]
    z[:, :, 0] = 0.0  # branch 0 IS the mean
    return z


def restate_samples(mean, std, noise) -> np.ndarray:
    """x = (float)min(max(mean + std * z, -1), 1): mean / std [E, K, size], noise [E, B, K, size] -> f32 [E, B, K, size]."""
    d = np.asarray(std, F64)[:, None] * np.asarray(noise, F64)
    y = np.asarray(mean, F64)[:, None] + d
    return np.minimum(np.maximum(y, -1.0), 1.0).astype(F32)


def score_key(g) -> np.ndarray:
    """csrc/hwy_lookahead.h: score_key, the order-preserving integer key of a double."""
    bits = np.asarray(g, F64).view(np.uint64)
    return np.where(bits >> np.uint64(63), ~bits, bits | np.uint64(1 << 63))


def elites_of(ret, M: int) -> np.ndarray:
    """The elite branches of one environment in ascending order: rank(b) = #{b': key' > key or (key' == key and b' < b)} < M."""
    keys = [int(k) for k in score_key(ret)]
    order = sorted(range(len(keys)), key=lambda b: (-keys[b], b))
    return np.asarray(sorted(order[:M]), np.int64)


def restate_refit(x, mean, std, alpha: float, min_std: float):
    """x f32 [M, K, size]: the elites' sequences in ascending branch order.  One rounded float64 operation per statement."""
    M = x.shape[0]
    xs = x.astype(F64)
    total = np.zeros(x.shape[1:])
    for j in range(M):
        total = total + xs[j]
    m = total / F64(M)
    acc = np.zeros(x.shape[1:])
    for j in range(M):
        d = xs[j] - m
        q = d * d
        acc = acc + q
    v = acc / F64(M)
    s = np.sqrt(v)
    keep = F64(1.0) - F64(alpha)
    m_new = F64(alpha) * m
    m_old = keep * np.asarray(mean, F64)
    s_new = F64(alpha) * s
    s_old = keep * np.asarray(std, F64)
    s_mix = s_new + s_old
    return m_new + m_old, np.maximum(F64(min_std), s_mix)


def restate_plan(noise, returns_of, cem: _abi.HwyCemParams, init_mean=None) -> dict:
    """The whole search in NumPy given the noise [I, E, B, K, size] and ``returns_of(samples f32 [E, B, K, size]) -> f64 [E, B]``
    (the simulator): every iteration's samples, returns and elite set, the final mean / std, the best sequence and return, the action."""
    I, E, B, K, size = noise.shape
    mean = np.zeros((E, K, size)) if init_mean is None else np.array(init_mean, F64, copy=True)
    std = np.full((E, K, size), F64(cem.init_std))
    best_ret, best_seq = np.zeros(E), np.zeros((E, K, size), F32)
    out = {"samples": [], "returns": [], "elites": [], "best_return_per_iteration": []}
    for i in range(I):
        x = restate_samples(mean, std, noise[i])
        ret = np.asarray(returns_of(x), F64)
        new_mean, new_std, elites = np.empty_like(mean), np.empty_like(std), []
        for e in range(E):
            el = elites_of(ret[e], cem.elites)
            elites.append(el)
            new_mean[e], new_std[e] = restate_refit(x[e][el], mean[e], std[e], cem.alpha, cem.min_std)
            top = elites_of(ret[e], 1)[0]
            if i == 0 or int(score_key(ret[e, top])) > int(score_key(best_ret[e])):
                best_ret[e], best_seq[e] = ret[e, top], x[e, top]
        mean, std = new_mean, new_std
        out["samples"].append(x); out["returns"].append(ret); out["elites"].append(elites)
        out["best_return_per_iteration"].append(best_ret.copy())
    out.update(samples=np.stack(out["samples"]), mean=mean, std=std, best_sequence=best_seq, best_return=best_ret, action=best_seq[:, 0].copy())
    return out


def fold_returns(reward, terminated, truncated, gamma: float) -> np.ndarray:
    """The score kernel's recurrence in NumPy: reward [..., K(, A)], flags [..., K] -> returns [...(, A)]; an ended episode is absorbing."""
    reward = np.asarray(reward, F64)
    agents = reward.ndim == np.ndim(terminated) + 1
    K = reward.shape[-2] if agents else reward.shape[-1]
    g = np.zeros(reward.shape[:-2] + reward.shape[-1:] if agents else reward.shape[:-1])
    alive = np.ones(np.shape(terminated)[:-1], bool)
    d = F64(1.0)
    for k in range(K):
        r = reward[..., k, :] if agents else reward[..., k]
        t = d * r
        live = alive[..., None] if agents else alive
        g = np.where(live, g + t, g)
        alive = alive & ~(np.asarray(terminated)[..., k] | np.asarray(truncated)[..., k])
        d = d * F64(gamma)
    return g


def assert_bits_equal(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=what)


def parent_snapshot(env) -> dict:
    eng = env._engine
    snap = {k: np.array(v, copy=True) for k, v in eng.get_state().items()}
    acc, steer = eng.get_controls()
    snap["ctl_accel"], snap["ctl_steer"] = acc.copy(), steer.copy()
    return snap


def assert_parent_unchanged(env, snap: dict):
    now = parent_snapshot(env)
    for k, v in snap.items():
        assert_bits_equal(now[k], v, f"parent {k}")


# ---- fixtures of tests/golden/cem ------------------------------------------------------------------------------------------------------
FIXTURES = ["cem_crash", "cem_respawn", "cem_ma2", "cem_longi_only"]
REWARD_ATOL = 1e-9   # tests/golden_util.py's tolerance for rewards (the project's standing one)


def _golden_base():
    from tests.lookahead_util import LookaheadGolden
    return LookaheadGolden


class CemGolden(_golden_base()):
    """A fixture of tests/golden/cem: make_golden_cem.py's record of ``copy.deepcopy(env)`` + ``env.step`` with ``ContinuousAction``.
    ``config["action"]`` is the matching ``DiscreteAction`` dict (what the engine is configured with); ``sequences`` are float32
    [B, K, A, size]."""

    def __init__(self, name: str):
        from tests.continuous_util import discrete_of, params_of
        with np.load(os.path.join(CEM_DIR, name + ".npz")) as z:
            data = {k: z[k] for k in z.files}
        super().__init__(name, data)
        self.sequences = np.asarray(data["sequences"], np.float32)
        self.ref_action = json.loads(str(data["cfg_action_json"]))
        self.config["action"] = discrete_of(self.ref_action)
        self.config["observation"] = json.loads(str(data["cfg_observation_json"]))
        self.params = params_of(self.ref_action)

    def prev_state(self) -> dict:
        return self.state("prev", time=self.z["prev_time"])

    def controls_of(self, prefix: str, cfg):
        agents = [cfg.agent_index[a] for a in range(cfg.num_agents)]
        return (np.ascontiguousarray(self.z[prefix + "_act_accel"][:, agents]), np.ascontiguousarray(self.z[prefix + "_act_steering"][:, agents]))

    def branch_planes(self) -> np.ndarray:
        """The rollout's action planes f32 [K, E * B, A, size] (environment e * B + b is branch b of group e)."""
        B, K, A, size = self.sequences.shape
        return np.ascontiguousarray(np.broadcast_to(self.sequences.transpose(1, 0, 2, 3)[:, None], (K, self.E, B, A, size)).reshape(K, self.E * B, A, size))
