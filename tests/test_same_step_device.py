"""hwy_step_same_step_device: gymnasium's SameStep autoreset in one call, held to the next-step auto-reset it must agree with.

* one call against two -- engine X takes step(a), a snapshot and one more step (whose launch re-spawns what ended); engine Y takes
  ONE same-step call: the final planes are X's first-call rows, what Y keeps for the environments that ended is what X keeps after
  its second call, reward / terminated / truncated stay the first call's, and the environments that did not end are X after the first
  call, their final rows untouched (tests/same_step_util.py: one_call_against_two has the list), on every configuration of CONFIGS;
* the same episodes over twenty calls -- with actions a function of (environment, episode, step) the two modes return the same
  useful steps, terminal observations and first observations, bit for bit;
* what the entry point refuses.
The CPU runs are the emulation's (tests/emu/emu_same_step.py: the product's kernels, launch rules and sequence); the ``hip`` runs
are the product on the MI355X, held to the same properties."""
import numpy as np
import pytest

from highwayenv_amd import _abi
from tests import same_step_util as ssu
from tests.backends import BACKENDS


@pytest.mark.parametrize("name", sorted(ssu.CONFIGS))
@pytest.mark.parametrize("backend", BACKENDS)
def test_one_call_against_two(backend, name):
    n_term = n_trunc = 0
    for seed, warmup, action, stagger in ssu.ENTRIES[name]:
        t, u = ssu.one_call_against_two(backend, name, seed, warmup, action, stagger)
        n_term, n_trunc = n_term + t, n_trunc + u
    print(f"{name}: {n_term} episodes ended by terminated, {n_trunc} by truncated alone")
    assert n_term > 0, f"{name}: no compared episode ended by `terminated`"
    if name in ssu.BOTH_KINDS:
        assert n_trunc > 0, f"{name}: no compared episode ended by `truncated`"


@pytest.mark.parametrize("name,seed", [("fast", 1), ("v0_2agents", 2), ("merge", 3)])
@pytest.mark.parametrize("backend", BACKENDS)
def test_same_episodes_over_many_calls(backend, name, seed):
    n_term, n_trunc = ssu.assert_same_episodes(backend, name, seed, calls=20)
    print(f"{name}: {n_term} episodes ended by terminated, {n_trunc} by truncated alone")
    assert n_term > 0, f"{name}: no episode ended by `terminated`"
    if name in ssu.BOTH_KINDS:
        assert n_trunc > 0, f"{name}: no episode ended by `truncated`"


# ---- refusals (the product's own validation, csrc/hwy_same_step.h: same_step_validate, through the emulated engine) -----------------
def _engine(cfg, autoreset=True):
    eng = ssu.make_engine("emu", cfg)
    eng.reset(seeds=np.arange(cfg.num_envs, dtype=np.uint64))
    if autoreset:
        eng.set_autoreset(True, base_seed=1)
    return eng


def _status(eng, **kw):
    from tests.emu import emu
    L, c = emu.lib("same_step"), eng.cfg
    import ctypes as C
    return L.emu_same_step_validate(C.byref(c), int(eng.autoreset[0]), int(kw.get("final_obs", 1)), int(kw.get("final_mask", 1)),
                                    int(kw.get("masks", 0)))


def test_intersection_is_unsupported():
    from highwayenv_amd import intersection
    cfg = _abi.make_config(intersection.intersection_default_config(), 2, scenario="intersection")
    eng = ssu.make_engine("emu", cfg)
    eng.set_autoreset(True, base_seed=1)
    assert _status(eng) == _abi.HWY_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError, match="intersection"):
        eng.step_same_step(np.ones((2, cfg.num_agents), np.int32))


def test_autoreset_must_be_enabled():
    from highwayenv_amd.engine import EngineError
    eng = _engine(ssu.config("fast"), autoreset=False)
    assert _status(eng) == _abi.HWY_ERR_INVALID_ARG
    with pytest.raises(EngineError, match="auto-reset must be enabled"):
        eng.step_same_step(np.ones((8, 1), np.int32))


@pytest.mark.parametrize("plane", ["final_obs", "final_mask"])
def test_null_final_plane_is_refused(plane):
    from highwayenv_amd.engine import EngineError
    eng = _engine(ssu.config("fast"))
    assert _status(eng, **{plane: 0}) == _abi.HWY_ERR_INVALID_ARG
    before = ssu.full_state(eng)
    with pytest.raises(EngineError, match="non-NULL"):
        eng.step_same_step(np.ones((8, 1), np.int32), without=(plane,))
    after = ssu.full_state(eng)
    for k in before:  # refused before any launch
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)


def test_mask_pointers_on_a_discrete_action_engine():
    """Refused as hwy_action_mask_device refuses them: HWY_ERR_UNSUPPORTED, the project's NotImplementedError."""
    from tests.emu import emu
    eng = _engine(ssu.config("direct"))
    assert _status(eng, masks=1) == emu.mask_status(eng.cfg) == _abi.HWY_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError, match="DiscreteMetaAction"):
        eng.step_same_step(np.zeros((4, 1), np.int32), masks=True)
    assert _status(eng, masks=0) == _abi.HWY_OK
    eng.step_same_step(np.zeros((4, 1), np.int32))  # (without them the call runs)


@pytest.mark.gpu
def test_refusals_of_the_library():
    """The same statuses from libhwy_engine.so on the device."""
    from highwayenv_amd.engine import EngineError
    eng = ssu.make_engine("hip", ssu.config("fast"))
    try:
        eng.reset(seeds=np.arange(8, dtype=np.uint64))
        with pytest.raises(EngineError, match="auto-reset must be enabled"):
            eng.step_same_step(np.ones((8, 1), np.int32))
        eng.set_autoreset(True, base_seed=1)
        for plane in ("final_obs", "final_mask"):
            with pytest.raises(EngineError, match="non-NULL"):
                eng.step_same_step(np.ones((8, 1), np.int32), without=(plane,))
    finally:
        eng.close()
    direct = ssu.make_engine("hip", ssu.config("direct"))
    try:
        direct.reset(seeds=np.arange(4, dtype=np.uint64))
        direct.set_autoreset(True, base_seed=1)
        with pytest.raises(NotImplementedError, match="DiscreteMetaAction"):
            direct.step_same_step(np.zeros((4, 1), np.int32), masks=True)
    finally:
        direct.close()
    from highwayenv_amd import intersection
    ix = ssu.make_engine("hip", _abi.make_config(intersection.intersection_default_config(), 2, scenario="intersection"))
    try:
        ix.set_autoreset(True, base_seed=1)
        with pytest.raises(NotImplementedError, match="intersection"):
            ix.step_same_step(np.ones((2, ix.cfg.num_agents), np.int32))
    finally:
        ix.close()
