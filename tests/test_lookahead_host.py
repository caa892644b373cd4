"""Environment fork / scoring of action sequences on the host side: the additive ABI, what the entry points accept and refuse
(shared validation of csrc/hwy_lookahead.h, through the CPU emulation and, marked ``gpu``, through the engine), the Python errors of
``fork`` / ``score_sequences`` / ``plan_lookahead``, and the fixtures of tests/golden/lookahead against their manifest."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from highwayenv_amd import _abi, _lib, envs, intersection, merge
from tests import lookahead_util as lu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECT = {"type": "DiscreteAction", "steering_range": [-0.1, 0.1]}


def _cfg(n=8, envs_=3, **over):
    return _abi.make_config(lu.highway_config(n, **over), envs_, fast=True)


def _other_scenarios():
    return {"merge": _abi.make_config(merge.merge_default_config(), 2, scenario="merge"),
            "merge-generic": _abi.make_config(merge.merge_generic_default_config(), 2, scenario="merge-generic"),
            "intersection": _abi.make_config(dict(intersection.intersection_default_config(), host_traffic=False), 2, scenario="intersection")}


def test_abi_is_additive():
    from tests.emu import emu
    lib = _lib.load()
    assert lib.hwy_abi_version() == _abi.HWY_ABI_VERSION == 8
    assert lib.hwy_config_size() == C.sizeof(_abi.HwyConfig) == emu.lib("lookahead").emu_lookahead_config_size() == 6304
    header = open(os.path.join(ROOT, "include", "hwy_engine.h")).read()
    assert "#define HWY_ABI_VERSION 8" in header
    for name in ("hwy_fork_device", "hwy_fork", "hwy_score_device", "hwy_score_rollout"):
        assert name in _lib.EXPORTS and name in header
    assert lib.hwy_fork_device(None, None, 1, None) == _abi.HWY_ERR_INVALID_ARG
    assert lib.hwy_fork(None, None, 1, None) == _abi.HWY_ERR_INVALID_ARG
    assert lib.hwy_score_device(None, 1, 1, 1.0, *([None] * 8)) == _abi.HWY_ERR_INVALID_ARG
    assert lib.hwy_score_rollout(None, 1, 1, 1.0, *([None] * 8)) == _abi.HWY_ERR_INVALID_ARG
    from highwayenv_amd import build
    kernels = build.kernel_resources()
    for name in ("hwy::hwy_fork_kernel<256>", "hwy::hwy_score_kernel<256>"):
        assert kernels[name]["vgpr_spill"] == 0 and kernels[name]["scratch"] == 0


def test_fork_validation_statuses():
    """fork_validate: the statuses hwy_fork_device returns before any launch."""
    from tests.emu.emu import fork_status
    src = _cfg()
    assert fork_status(lu.with_envs(src, 6), src, branches=2) == 0
    assert fork_status(lu.with_envs(src, 5), src, branches=1, has_source=True) == 0          # any size with source indices
    tuned = lu.with_envs(src, 6)
    tuned.tune_waves_per_eu, tuned.tune_prio_shift = 4, -1
    assert fork_status(tuned, src, branches=2) == 0                                           # tune_* may differ
    bad = _abi.HWY_ERR_INVALID_ARG
    assert fork_status(src, src, same_engine=True) == bad
    assert fork_status(lu.with_envs(src, 6), src, branches=0) == bad
    assert fork_status(lu.with_envs(src, 7), src, branches=2) == bad                          # 7 != 3 * 2
    assert fork_status(lu.with_envs(_cfg(9), 6), src, branches=2) == bad                      # another N
    assert fork_status(lu.with_envs(_cfg(duration=7), 6), src, branches=2) == bad             # another duration
    assert fork_status(lu.with_envs(_cfg(action=DIRECT), 6), src, branches=2) == bad          # another ego control
    for name, other in _other_scenarios().items():
        assert fork_status(lu.with_envs(other, 4), other, branches=2) == _abi.HWY_ERR_UNSUPPORTED, name
        assert fork_status(lu.with_envs(src, 6), other, branches=2) == _abi.HWY_ERR_UNSUPPORTED, name


def test_score_validation_statuses():
    from highwayenv_amd.engine import EngineError
    from tests.emu import emu
    cfg = _cfg(envs_=6)
    r, f, a = np.zeros((2, 6, 1)), np.zeros((2, 6), np.uint8), np.zeros((6, 1), np.int32)
    emu.score(cfg, 2, 3, 0.9, a, r, f, f)
    emu.score(cfg, 2, 3, 0.9, None, r, f, f, want=("returns", "best_branch"))
    for kw in (dict(k_steps=0), dict(branches=0), dict(branches=4), dict(gamma=np.inf), dict(gamma=np.nan), dict(reward=None),
               dict(terminated=None), dict(first_action=None), dict(want=("returns",))):
        args = dict(k_steps=2, branches=3, gamma=0.9, first_action=a, reward=r, terminated=f, truncated=f)
        want = kw.pop("want", ("returns", "q", "best_action", "best_branch"))
        args.update(kw)
        with pytest.raises(EngineError, match=f"status {_abi.HWY_ERR_INVALID_ARG}:"):
            emu.score(cfg, want=want, **args)
    two = _abi.make_config(lu.highway_config(8, controlled_vehicles=2, action={"type": "MultiAgentAction", "action_config": {"type": "DiscreteMetaAction"}},
                                             observation={"type": "MultiAgentObservation", "observation_config": {"type": "Kinematics"}}), 6, fast=True)
    r2, a2 = np.zeros((2, 6, 2)), np.zeros((6, 2), np.int32)
    emu.score(two, 2, 3, 0.9, None, r2, f, f, want=("returns", "best_branch"))
    for want in (("q",), ("best_action",)):   # A > 1
        with pytest.raises(EngineError, match="single agent"):
            emu.score(two, 2, 3, 0.9, a2, r2, f, f, want=want)
    for name, other in _other_scenarios().items():
        with pytest.raises(NotImplementedError, match="hot-path scope"):
            emu.score(other, 1, 1, 1.0, None, np.zeros((1, 2, other.num_agents)), np.zeros((1, 2), np.uint8), np.zeros((1, 2), np.uint8),
                                want=("returns",))


@pytest.mark.gpu
def test_engine_entry_points_refuse_mismatched_engines_and_other_scenarios():
    from highwayenv_amd.engine import Engine, EngineError
    src = _cfg()
    parent, child, other_n = Engine(src), Engine(lu.with_envs(src, 6)), Engine(lu.with_envs(_cfg(9), 6))
    parent.reset()
    child.fork_from(parent, 2)
    child.fork_from(parent, 1, source=[0, 2, 1, 1, 0, 2])
    for call in (lambda: parent.fork_from(parent, 1), lambda: child.fork_from(parent, 3), lambda: other_n.fork_from(parent, 2),
                 lambda: child.fork_from(parent, 1, source=[0, 1, 2, 3, 0, 0]), lambda: child.fork_from(parent, 1, source=[0, -1, 2, 1, 0, 0]),
                 lambda: child.score_device(2, 4, 0.9, 0, 1, 1, 1), lambda: child.score_device(0, 2, 0.9, 0, 1, 1, 1),
                 lambda: child.score_device(2, 2, 0.9, 0, 0, 1, 1), lambda: child.score_device(2, 2, 0.9, 0, 1, 1, 1, d_q=1)):
        with pytest.raises(EngineError, match="invalid argument"):
            call()
    with pytest.raises(KeyError):
        child.score_rollout(np.full((2, 6, 1), 5, np.int32), 2)
    for eng in (parent, child, other_n):
        eng.close()
    for name, cfg in _other_scenarios().items():
        a, b = Engine(cfg), Engine(cfg)
        for call in (lambda: a.fork_from(b, 1), lambda: a.score_device(1, 1, 1.0, 0, 1, 1, 1),
                     lambda: a.score_rollout(np.zeros((1, cfg.num_envs, cfg.num_agents), np.int32), 1)):
            with pytest.raises(NotImplementedError, match="hot-path scope"):
                call()
        a.close(), b.close()


@pytest.mark.parametrize("cls", [envs.BatchedMergeEnv, envs.BatchedMergeGenericEnv, envs.BatchedIntersectionEnv])
def test_python_raises_not_implemented_off_the_highway(cls):
    env = cls(num_envs=2)
    for call in (lambda: env.fork(2), lambda: env.score_sequences([[1, 1]]), lambda: env.plan_lookahead(1)):
        with pytest.raises(NotImplementedError, match="hot-path scope"):
            call()


def test_python_errors_on_the_highway():
    cls = lu.env_class("emu")
    env = cls(lu.highway_config(8), num_envs=2, spawn_mode="device")
    for call in (lambda: env.fork(), lambda: env.score_sequences([[1, 1]]), lambda: env.plan_lookahead(1)):
        with pytest.raises(NotImplementedError, match="must be initialized"):   # before reset(), like step
            call()
    env.reset(seed=1)
    with pytest.raises(ValueError, match="horizon"):
        env.plan_lookahead(2, horizon=1)
    with pytest.raises(ValueError, match="depth"):
        env.plan_lookahead(0)
    with pytest.raises(ValueError, match="branches"):
        env.fork(0)
    with pytest.raises(ValueError, match="source"):
        env.fork(1, source=[0, 2])
    with pytest.raises(ValueError, match="shape"):
        env.score_sequences(np.zeros((3, 2, 2, 2, 2), np.int64))
    with pytest.raises(KeyError):
        env.score_sequences([[1, 5]])
    env.max_fork_bytes = 100_000
    with pytest.raises(ValueError, match=r"\d+ bytes"):   # 2 * 5 ** 3 environments do not fit: the bytes needed are named
        env.plan_lookahead(3)
    assert _abi.fork_bytes(env._hcfg, 250, 3) > 100_000
    env.max_fork_bytes = None
    with pytest.raises(ValueError, match="do not fit"):
        env.plan_lookahead(14)   # 5 ** 14 branches
    env.close()
    two = cls(lu.highway_config(8, controlled_vehicles=2, action={"type": "MultiAgentAction", "action_config": {"type": "DiscreteMetaAction"}},
                                observation={"type": "MultiAgentObservation", "observation_config": {"type": "Kinematics"}}),
              num_envs=2, spawn_mode="device")
    two.reset(seed=1)
    with pytest.raises(NotImplementedError, match="single agent"):
        two.plan_lookahead(1)
    assert two.score_sequences(np.ones((3, 2, 2), np.int64)).shape == (2, 3, 2)   # score_sequences serves several agents
    two.close()
    direct = cls(lu.highway_config(8, action=DIRECT), num_envs=2, spawn_mode="device")
    direct.reset(seed=1)
    with pytest.raises(NotImplementedError, match="DiscreteMetaAction"):
        direct.plan_lookahead(1)
    with pytest.raises(IndexError):
        direct.score_sequences([[9, 0]])
    returns, details = direct.score_sequences(np.arange(8).reshape(4, 2), return_details=True)
    assert returns.shape == (2, 4) and details["q"].shape == (2, 9) and np.isneginf(details["q"][:, 1]).all()
    direct.close()


def test_lookahead_table_digits():
    env = lu.env_class("emu")(lu.highway_config(8), num_envs=1)
    t = env.lookahead_table(3, 5)
    assert t.shape == (125, 5) and t.dtype == np.int32
    np.testing.assert_array_equal(t[37], [1, 2, 2, 1, 1])   # 37 = 1 * 25 + 2 * 5 + 2, then IDLE
    np.testing.assert_array_equal(t[:, 0] * 25 + t[:, 1] * 5 + t[:, 2], np.arange(125))
    assert env.lookahead_table(3, 5) is t   # built once
    lat = lu.env_class("emu")(lu.highway_config(8, action={"type": "DiscreteMetaAction", "longitudinal": False}), num_envs=1)
    assert lat.lookahead_table(2).shape == (9, 2)


def test_single_env_drop_in_plans():
    """The E == 1 drop-in offers the same calls (its child is the batched class)."""
    from tests.emu.emu import EmuEngine

    class Emu(envs.HighwayEnvFast):
        _engine_factory = staticmethod(lambda cfg, device, stream: EmuEngine(cfg))
    env = Emu(lu.highway_config(8))
    best = env.plan_lookahead(2)
    assert best.shape == (1,) and 0 <= int(best[0]) < 5
    env.step(int(best[0]))
    env.close()


def test_fixture_digests_match_the_manifest():
    import hashlib
    manifest = json.load(open(os.path.join(lu.DIR, "MANIFEST.json")))
    assert sorted(manifest) == sorted(lu.FIXTURES)
    for name in lu.FIXTURES:
        path = os.path.join(lu.DIR, name + ".npz")
        assert os.path.getsize(path) < 1 << 20
        with np.load(path) as z:
            h = hashlib.sha256()
            for k in sorted(z.files):
                a = np.asarray(z[k])
                h.update(k.encode())
                h.update(str(a.dtype).encode() + str(a.shape).encode())
                h.update(np.ascontiguousarray(a).tobytes())
        assert h.hexdigest() == manifest[name], f"{name}.npz is not what make_golden_lookahead.py recorded"
