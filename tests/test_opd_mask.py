"""The masked optimistic planner (``plan_opd(masked=True)``, HWY_OPD_MASKED): the search equals its plain Python restatement
(tests/opd_mask_util.py) bit for bit -- on the CPU emulation of the kernels and, marked ``gpu``, on the MI355X, where it also equals
the emulation --, an all-true mask gives the unmasked search, no action of a returned sequence is unavailable in the state it is
applied to, the parent is left as it was, unknown ``flags`` bits are refused, and the front ends pass the flag through."""
import numpy as np
import pytest

from highwayenv_amd import _abi
from tests import opd_mask_util as omu
from tests.lookahead_util import with_envs
from tests.opd_mask_util import BACKENDS

# 3 lanes with 3 speeds, 1 lane, 2 speeds: 20 vehicles, E = 3; warmed towards an edge lane and an end of the speed ladder
SHAPES = {"lanes3_speeds3": dict(vehicles_count=19), "lane1": dict(vehicles_count=19, lanes_count=1),
          "speeds2": dict(vehicles_count=19, action={"type": "DiscreteMetaAction", "target_speeds": [20.0, 28.0]})}
WARM = ([0, 2, 3], [0, 2, 4])


def _env(backend, shape, seed=5):
    return omu.make_env(backend, omu.fast_config(**{k: v for k, v in SHAPES[shape].items()}), 3, seed, warm=WARM)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("budget", [5, 15, 50])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_masked_search_equals_its_restatement(shape, budget, backend):
    env = _env(backend, shape)
    before = env.get_state()
    want = omu.restate_masked_opd(backend, env, budget, 0.7)
    action, got = env.plan_opd(budget, 0.7, return_details=True, masked=True)
    omu.assert_plan_equals(action, got, want, f"{shape} budget {budget}")
    after = env.get_state()
    assert all(np.array_equal(before[k], after[k]) for k in before)        # the parent is left bit for bit as it was
    if budget >= 15:
        assert want["masked_out"].sum() > 0                                 # the mask took children away somewhere
    if shape == "lane1":
        assert not np.isin(got["sequence"], (0, 2)).any()                   # one lane: no lane change anywhere in a plan
    if backend == "hip" and budget >= 15:                                   # ... and the HIP search equals the emulated one
        emu_env = omu.env_class("emu")(env.config, num_envs=3)
        emu_env.reset(seed=0)
        emu_env.set_state(before)
        a2, g2 = emu_env.plan_opd(budget, 0.7, return_details=True, masked=True)
        omu.assert_plan_equals(a2, g2, want, f"{shape} budget {budget}: emulator")
        emu_env.close()
    env.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_all_true_mask_equals_the_unmasked_search(backend):
    """Ego in a middle lane at the middle speed, budget = n_ids: every action of the one expanded node is available."""
    env = omu.make_env(backend, omu.fast_config(19, initial_lane_id=1), 3, 7)
    assert env.get_available_actions().all()
    a0, d0 = env.plan_opd(5, 0.7, return_details=True)
    a1, d1 = env.plan_opd(5, 0.7, return_details=True, masked=True)
    omu.assert_plan_equals(a1, d1, dict(d0, action=a0), "all-true mask")
    env.close()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", ["lanes3_speeds3", "speeds2"])
def test_no_unavailable_action_in_a_returned_sequence(shape, backend):
    env = _env(backend, shape, seed=9)
    _, d = env.plan_opd(50, 0.7, return_details=True, masked=True)
    assert omu.replay_is_available(backend, env, d["sequence"]) >= 3 * 2
    # the unmasked search is what the masks are for: from an edge lane it offers actions the reference does not
    env.close()


def test_unknown_flags_bits_are_rejected():
    from tests.emu import emu
    cfg = _abi.make_config(omu.fast_config(8), 2, fast=True)
    p = _abi.opd_params(cfg, 15, 0.7)
    tree, work = with_envs(cfg, 2 * p.nodes), with_envs(cfg, 2 * p.n_ids)
    assert emu.opd_validate(cfg, tree, work, p) == 0
    p.flags = _abi.HWY_OPD_MASKED
    assert emu.opd_validate(cfg, tree, work, p) == 0
    for bad in (2, 3, 4, 1 << 30, -1):
        p.flags = bad
        assert emu.opd_validate(cfg, tree, work, p) == _abi.HWY_ERR_INVALID_ARG, bad
    direct = _abi.make_config(omu.fast_config(8, action={"type": "DiscreteAction"}), 2, fast=True)
    q = _abi.opd_params(direct, 18, 0.7, masked=True)
    assert emu.opd_validate(direct, with_envs(direct, 2 * q.nodes), with_envs(direct, 2 * q.n_ids), q) == _abi.HWY_ERR_UNSUPPORTED
    q.flags = 0
    assert emu.opd_validate(direct, with_envs(direct, 2 * q.nodes), with_envs(direct, 2 * q.n_ids), q) == 0


@pytest.mark.gpu
def test_unknown_flags_bits_are_rejected_by_the_engine():
    from highwayenv_amd.engine import EngineError
    env = omu.make_env("hip", omu.fast_config(8), 2, 1)
    params, tree, work = env._opd_setup(15, 0.7)
    params.flags = 2
    with pytest.raises(EngineError):
        env._engine.opd_plan(tree._engine, work._engine, params)
    env.close()


@pytest.mark.gpu
def test_step_on_the_masked_plan_never_leaves_the_device():
    import torch

    from highwayenv_amd.vector import HighwayVectorEnv
    venv = HighwayVectorEnv("highway-fast-v0", num_envs=4, config={"vehicles_count": 12}, output="torch", action_masks=True)
    _, info = venv.reset(seed=2)
    for t in range(5):
        mask = info["action_mask"].clone()
        action = venv.plan_opd(15, 0.7, masked=True)
        assert isinstance(action, torch.Tensor) and action.is_cuda and action.dtype == torch.int32
        assert bool(mask[torch.arange(4, device=mask.device), action.long()].all())   # the first action is available now
        _, _, _, _, info = venv.step(action)
    venv.close()
