"""The step kernels compiled for the registered configurations (csrc/hwy_wave.h: FixedShape) against the REFERENCE's recorded episodes.

tests/test_engine_parity.py: test_free_running_episodes_vs_reference runs the fixtures of tests/golden without auto-reset, i.e. on
the generic kernel (csrc/hwy_launch_family.h: step_shape_of).  Here the fixtures whose configuration is a registered shape run
again with auto-reset switched on after ``set_state``, so that every launch takes the shape's kernel -- asserted at every step --
at that test's tolerances: observation 1e-6, reward and speed 1e-9, state 1e-7, lanes / flags / terminated / truncated exact.

That test re-synchronises an environment from the fixture once it holds a wreck.  Under auto-reset the device re-spawns an ended
environment on the next step, so an environment is compared up to and including the step in which it ends or first holds a wreck
and is dropped from there on (environments are independent: the others are unaffected).  The number of env-steps compared must be
what the same rule counts on the fixture alone: nothing is dropped silently."""
import numpy as np
import pytest

from highwayenv_amd import _abi
from tests import variants_util as vu
from tests.backends import BACKENDS, make_engine
from tests.golden_util import ALL, Golden, assert_state_close


def _shape_of(name: str) -> int:
    g = Golden(name)
    return vu.step_shape(g.config, {"fast": g.fast})


SHAPED = {name: _shape_of(name) for name in ALL if _shape_of(name)}


def test_the_fixtures_cover_every_shape():
    assert set(SHAPED.values()) == set(vu.SHAPES), SHAPED
    assert {"cfg1_fast_default", "cfg2_fast_n50_l4", "v0_default"} <= set(SHAPED), SHAPED
    # (dense_crash is highway-v0 on THREE lanes and cfg3_v0_n100 holds 101 vehicles: no shape, the generic kernels run them)
    assert "dense_crash" not in SHAPED and "cfg3_v0_n100" not in SHAPED


def _wreck(g, t):
    want = g.state("step", t, time=float(t + 1))
    return want, ((want["flags"] & (_abi.F_CRASHED | _abi.F_HAS_IMPACT)) != 0).any(1)


def fixture_env_steps(g) -> int:
    """The env-steps compared in full, counted on the fixture alone: an environment counts while it is live and collision-free in
    the step (the rule of test_free_running_episodes_vs_reference), up to its end -- terminated, truncated or a first wreck."""
    live, n = np.ones(g.E, bool), 0
    for t in range(g.steps):
        _, wreck_now = _wreck(g, t)
        n += int((live & ~wreck_now).sum())
        live = live & ~wreck_now & ~g.z["terminated"][t].astype(bool) & ~g.z["truncated"][t].astype(bool)
    return n


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", list(SHAPED))
def test_free_running_episodes_vs_reference_on_the_shape_kernel(backend, name):
    g = Golden(name)
    cfg = _abi.make_config(g.config, g.E, fast=g.fast)
    eng = make_engine(backend, cfg)
    try:
        eng.set_state(g.state("init"))
        eng.set_autoreset(True, base_seed=11, ego_spacing=g.config["ego_spacing"], vehicles_density=g.config["vehicles_density"])
        np.testing.assert_allclose(eng.observe()[:, 0], g.z["obs0"], rtol=0, atol=1e-6)
        live = np.ones(g.E, bool)
        compared = 0
        for t in range(g.steps):
            obs, reward, term, trunc, info = eng.step(g.actions[t])
            what = f"{name} step {t}"
            assert vu.last_step_shape(eng) == SHAPED[name], f"{what}: the launch ran shape {vu.last_step_shape(eng)}"
            want, wreck_now = _wreck(g, t)
            T_ = live              # episodes live at the start of the step: flags / termination / reward
            L = live & ~wreck_now  # ... and collision-free during it: everything
            compared += int(L.sum())
            np.testing.assert_array_equal(term[T_], g.z["terminated"][t].astype(bool)[T_], err_msg=what)
            np.testing.assert_array_equal(trunc[T_], g.z["truncated"][t].astype(bool)[T_], err_msg=what)
            np.testing.assert_array_equal(info["crashed"][T_, 0], g.z["info_crashed"][t].astype(bool)[T_], err_msg=what)
            np.testing.assert_allclose(reward[T_, 0], g.z["reward"][t][T_], rtol=0, atol=1e-6, err_msg=what)
            np.testing.assert_allclose(obs[L, 0], g.z["obs"][t][L], rtol=0, atol=1e-6, err_msg=what)
            np.testing.assert_allclose(reward[L, 0], g.z["reward"][t][L], rtol=0, atol=1e-9, err_msg=what)
            np.testing.assert_allclose(info["speed"][L, 0], g.z["info_speed"][t][L], rtol=0, atol=1e-9, err_msg=what)
            got = eng.get_state()
            assert_state_close({k: v[L] for k, v in got.items()}, {k: v[L] for k, v in want.items()}, atol=1e-7, what=what)
            # an ended environment is re-spawned by the next launch, a wreck that has not ended its episode rots: neither is compared again
            live = live & ~wreck_now & ~term & ~trunc
    finally:
        eng.close()
    assert compared == fixture_env_steps(g) > 0, (compared, fixture_env_steps(g))
