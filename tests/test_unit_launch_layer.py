"""The add-on units' launch layer (csrc/hwy_launch_units.h), the OPD sequence (csrc/hwy_opd.h: opd_expand) and the one emulated
engine (tests/emu/emu.py), on the CPU: what the emulation shares with the product it also REFUSES like the product, the sequence of
a plan is the product's, and one class simulates every configuration with the driver hwy_engine.hip's with_family picks."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from highwayenv_amd import _abi, intersection, merge
from highwayenv_amd.engine import EngineError
from tests import backends
from tests.emu import emu
from tests.emu.emu import _p

LINEAR = "highway_env.vehicle.behavior.LinearVehicle"
LIDAR = {"type": "LidarObservation"}
DIRECT = {"type": "DiscreteAction"}


def _config(E=2, **over) -> _abi.HwyConfig:
    return _abi.make_config(dict(_abi.highway_fast_default_config(), vehicles_count=1, normalize_reward=True, **over), E, fast=True)


def _copy(cfg, **fields) -> _abi.HwyConfig:
    out = _abi.HwyConfig.from_buffer_copy(bytes(cfg))
    for k, v in fields.items():
        setattr(out, k, v)
    return out


def _engine(cfg):
    eng = backends.make_engine("emu", cfg)
    eng.reset(base_seed=3)
    return eng


# ---- guards reach the emulation ----------------------------------------------------------------------------------------------------------
# Each launch goes to the unit's entry point BEHIND the validation (what EmuEngine calls after the product's *_validate has passed),
# with arguments just outside a precondition of the unit's rule in hwy_launch_units.h: the status is HWY_ERR_HIP, the product's for a
# refused launch, and nothing was written.
def test_lidar_rule_refuses_zero_cells():
    cfg = _config(observation=LIDAR)
    eng = _engine(cfg)
    obs = np.full((cfg.num_envs, 1, cfg.lidar_cells, 2), -3.0, np.float32)
    s = _abi.state_struct(eng.st)
    assert emu.lib("lidar").emu_lidar_observe(C.byref(_copy(cfg, lidar_cells=0)), C.byref(s), _p(obs, C.c_float)) == _abi.HWY_ERR_HIP
    assert (obs == -3.0).all()
    assert emu.lib("lidar").emu_lidar_observe(C.byref(cfg), C.byref(s), _p(obs, C.c_float)) == 0 and (obs != -3.0).all()


def test_ttc_rule_refuses_one_time_step_too_many():
    cfg = _config()
    eng = _engine(cfg)
    params = _abi.ttc_params(_abi.highway_fast_default_config(), horizon=6.4, time_quantization=0.1)
    assert params.time_steps == _abi.HWY_MAX_TTC_STEPS
    s = _abi.state_struct(eng.st)
    for plan in (0, 1):
        for steps, status in ((_abi.HWY_MAX_TTC_STEPS + 1, _abi.HWY_ERR_HIP), (_abi.HWY_MAX_TTC_STEPS, 0)):
            params.time_steps = steps
            grid = np.full((cfg.num_envs, 1, *emu.ttc_shape(cfg, params)), -3.0, np.float32)
            action = np.full((cfg.num_envs, 1), -3, np.int32)
            assert emu.lib("ttc").emu_ttc_launch(C.byref(cfg), C.byref(s), C.byref(params), plan, _p(grid, C.c_float), _p(action, C.c_int32),
                                                 None) == status
            if status:
                assert (grid == -3.0).all() and (action == -3).all()
            else:
                assert not (grid == -3.0).any() and (action == -3).all() == (not plan)


def test_score_rule_refuses_one_action_id_too_many():
    cfg = _config(action=DIRECT)
    reward, flags = np.ones((1, 2, 1)), np.zeros((1, 2), np.uint8)
    ret, branch = np.full((2, 1, 1), -3.0), np.full((2, 1), -3, np.int32)

    def launch(c):
        return emu.lib("lookahead").emu_lookahead_score(C.byref(c), C.c_int32(1), C.c_int32(1), C.c_double(0.9), None, _p(reward, C.c_double),
                                                        _p(flags, C.c_uint8), _p(flags, C.c_uint8), _p(ret, C.c_double), None, None,
                                                        _p(branch, C.c_int32))
    assert launch(_copy(cfg, n_accel=257, n_steer=1)) == _abi.HWY_ERR_HIP  # HWY_SCORE_MAX_IDS + 1
    assert (ret == -3.0).all() and (branch == -3).all()
    assert launch(_copy(cfg, n_accel=256, n_steer=1)) == 0 and (ret == 1.0).all() and (branch == 0).all()


def test_fork_rule_refuses_too_few_sources_without_indices():
    src, dst = _engine(_config(E=1)), _engine(_config(E=2))
    before = dst.get_state()
    (d, _d), (s, _s) = dst._view(), src._view()
    assert emu.lib("lookahead").emu_lookahead_fork(C.byref(d), C.byref(s), C.c_int32(1), None, 0) == _abi.HWY_ERR_HIP  # 1 * 1 < 2
    after = dst.get_state()
    assert all((before[k] == after[k]).all() for k in before)
    assert emu.lib("lookahead").emu_lookahead_fork(C.byref(d), C.byref(s), C.c_int32(2), None, 0) == 0
    assert (dst.get_state()["x"] == src.get_state()["x"][[0, 0]]).all()


def test_mask_rule_refuses_a_pitch_below_the_vehicles():
    cfg = _config()
    eng = _engine(cfg)
    mask = np.full((cfg.num_envs, 1, 5), 7, np.uint8)
    s = _abi.state_struct(eng.st)
    assert emu.lib("mask").emu_mask_launch(C.byref(cfg), C.byref(s), C.c_int(cfg.num_vehicles - 1), _p(mask, C.c_uint8)) == _abi.HWY_ERR_HIP
    assert (mask == 7).all()
    assert emu.lib("mask").emu_mask_launch(C.byref(cfg), C.byref(s), C.c_int(cfg.num_vehicles), _p(mask, C.c_uint8)) == 0 and (mask <= 1).all()


@pytest.mark.parametrize("what", ["nodes", "child_mask", "created"])
def test_opd_rule_refuses_a_wrong_node_count_and_half_a_masked_search(what):
    cfg = _config()
    params = _abi.opd_params(cfg, 10, 0.7, masked=what != "nodes")
    src, tree, work = (_engine(_copy(cfg, num_envs=n)) for n in (2, 2 * params.nodes, 2 * params.n_ids))
    before = tree.get_state()
    if what == "nodes":
        params.nodes += 1  # M != 1 + X * n
    with pytest.raises(EngineError, match="status -2"):
        src._opd_launch(tree, work, params, without=() if what == "nodes" else (what,))
    assert all((a == -7).all() for a in src.last_plan.values() if a.dtype == np.int32) and np.isnan(src.last_plan["value"]).all()
    assert (src.last_tree["actions"] == -7).all() and np.isnan(src.last_tree["ret"]).all()
    after = tree.get_state()
    assert all((before[k] == after[k]).all() for k in before)


# ---- the one sequence --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_opd_sequence_is_the_products(masked):
    """hwy_opd.h's opd_expand over recording operations, n = 5 action ids and X = 2 expansions: the order hwy_opd_plan_device has
    enqueued its launches in since the planner exists, with a stream-order operation before every kernel and before the root fork."""
    m = ["mask"] if masked else []
    want = (["after(work,tree)", "kernel(0)", "after(tree,work)", "fork(tree,src,1,root)", "fork(work,src,5,none)", *m, "step",
             "fork(tree,work,1,scatter)"]
            + ["after(work,tree)", "kernel(1)", "fork(work,tree,1,gather)", *m, "step", "fork(tree,work,1,scatter)"]
            + ["after(work,tree)", "kernel(2)"])
    assert emu.opd_sequence(5, 2, masked) == want


def test_emulated_plan_runs_that_sequence():
    """... and the emulated opd_plan is that template too: a plan of E = 2 with budget 10 (n = 5, X = 2) expands twice."""
    cfg = _config()
    for masked in (False, True):
        params = _abi.opd_params(cfg, 10, 0.7, masked=masked)
        src, tree, work = (_engine(_copy(cfg, num_envs=n)) for n in (2, 2 * params.nodes, 2 * params.n_ids))
        out = src.opd_plan(tree, work, params)
        assert out["expanded"].tolist() == [2, 2] and ((out["action"] >= 0) & (out["action"] < 5)).all()
        assert (src.last_tree["created"] != 0xff).any() == masked


# ---- the engine chooser ------------------------------------------------------------------------------------------------------------------
def _kinds():
    ix = dict(intersection.intersection_default_config(), max_vehicles=8, host_traffic=False)
    yield "IDM", _config(), "sim"
    yield "Linear", _config(other_vehicles_type=LINEAR), "traffic"
    yield "direct", _config(action=DIRECT), "control"
    yield "IDM Lidar", _config(observation=LIDAR), "sim"
    yield "Linear Lidar", _config(other_vehicles_type=LINEAR, observation=LIDAR), "traffic"
    yield "direct Lidar", _config(action=DIRECT, observation=LIDAR), "control"
    yield "merge", _abi.make_config(merge.merge_default_config(), 2, scenario="merge"), "sim"
    yield "intersection", _abi.make_config(ix, 2, scenario="intersection"), "sim"


@pytest.mark.parametrize("kind,cfg,family", [pytest.param(*k, id=k[0]) for k in _kinds()])
def test_one_engine_simulates_with_the_family_of_the_config(kind, cfg, family):
    """family: the kernel family hwy_engine.hip's with_family builds the arguments of -- the scenario first, then Linear traffic, then
    direct ego control; the Lidar trace goes behind it (launch_stage)."""
    eng = _engine(cfg)
    assert type(eng) is emu.EmuEngine and eng.family == family
    obs, reward, *_ = eng.step(np.ones((cfg.num_envs, cfg.num_agents), np.int32))
    assert obs.shape == (cfg.num_envs, cfg.num_agents, *_abi.obs_shape(cfg)) and np.isfinite(reward).all()
    assert (eng.extra is not None) == (family != "sim")
    # the units: they work, or raise what the product raises where its own validation says HWY_ERR_UNSUPPORTED
    params = _abi.ttc_params(_abi.highway_fast_default_config())
    other = _engine(cfg)
    calls = {"action_mask": (emu.mask_status(cfg), eng.action_mask),
             "ttc_grid": (emu.ttc_status(cfg, params), lambda: eng.ttc_grid(params)),
             "fork_from": (emu.fork_status(cfg, cfg), lambda: other.fork_from(eng))}
    scope = {"IDM": (0, 0, 0), "Linear": (0, 0, 0), "direct": (-3, -3, 0), "IDM Lidar": (0, 0, 0), "Linear Lidar": (0, 0, 0),
             "direct Lidar": (-3, -3, 0), "merge": (0, -3, -3), "intersection": (0, -3, -3)}[kind]
    assert tuple(status for status, _ in calls.values()) == scope
    for name, (status, call) in calls.items():
        if status == _abi.HWY_ERR_UNSUPPORTED:
            with pytest.raises(NotImplementedError):
                call()
        else:
            call()
    if scope[2] == 0:
        assert (other.get_state()["x"] == eng.get_state()["x"]).all()
