"""LidarObservation on the highway scenario (csrc/hwy_lidar.h: hwy_lidar_kernel, launched after the step / reset kernel of the
IDM, Linear and direct-control families) against the unmodified reference's fixtures (tests/golden/lidar), on the CPU emulation
of the kernel source (``emu``) and on the MI355X (``hip``).

The yardstick is the reference's own ``observe()``: recorded at reset and after every step of a run, and on the hand-placed
roads of ``lidar_crafted``.  Observations are compared at 1e-6, the project's observation tolerance, and the number of cells
beyond it is ZERO on every fixture (a cell differs grossly when an angle falls on the other side of a sector boundary: the
margins of the committed seeds are in tests/golden/lidar/README.md).  ``lidar_crafted`` -- ties, float32 rounding of the fold,
the range test on the centre, both wrap rules, headings exactly 0 -- is compared bit for bit."""
import numpy as np
import pytest

from highwayenv_amd import _abi
from tests.lidar_util import BACKENDS, FIXTURES, OBS_ATOL, RUNS, LidarGolden, cells_off, make_engine


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", FIXTURES)
def test_recorded_states(backend, name):
    """Every recorded state (reset, and after every step of the reference's run) loaded and observed: no cell beyond 1e-6."""
    g = LidarGolden(name)
    eng = make_engine(backend, g.hwy_config())
    off = total = 0
    worst = 0.0
    for index in [None] + list(range(g.steps)):
        g.load(eng, "init" if index is None else "step", index)
        got, want = eng.observe(), g.reference_obs(index)
        assert got.shape == want.shape and got.dtype == np.float32
        assert np.isfinite(got).all()
        off += cells_off(got, want)
        total += want[..., 0].size
        worst = max(worst, float(np.abs(got.astype(np.float64) - want).max()))
    eng.close()
    print(f"{name} [{backend}]: {off} of {total} cells beyond {OBS_ATOL}, largest difference {worst:.3g}")
    assert off == 0, f"{name}: {off} of {total} cells differ beyond {OBS_ATOL} (largest difference {worst:.3g})"


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", RUNS)
def test_free_running_episodes(backend, name):
    """Whole episodes from the reference's initial state: the lidar observation of every step at 1e-6 with no cell beyond it,
    reward 1e-9, terminated / truncated exact; each environment up to and including its first terminated step."""
    g = LidarGolden(name)
    eng = make_engine(backend, g.hwy_config())
    g.load(eng)
    np.testing.assert_allclose(eng.observe(), g.reference_obs(), rtol=0, atol=OBS_ATOL, err_msg=f"{name}: reset")
    alive = np.ones(g.E, bool)
    off = total = 0
    worst = 0.0
    for t in range(g.steps):
        obs, reward, term, trunc, info = eng.step(g.actions_at(t))
        rows = np.flatnonzero(alive)
        want = g.reference_obs(t)
        off += cells_off(obs[rows], want[rows])
        total += want[rows][..., 0].size
        worst = max(worst, float(np.abs(obs[rows].astype(np.float64) - want[rows]).max()) if len(rows) else 0.0)
        np.testing.assert_allclose(reward[rows, 0], g.z["reward"][t][rows], rtol=0, atol=1e-9, err_msg=f"{name} step {t}: reward")
        np.testing.assert_array_equal(term[rows], g.z["terminated"][t][rows].astype(bool), err_msg=f"{name} step {t}: terminated")
        np.testing.assert_array_equal(trunc[rows], g.z["truncated"][t][rows].astype(bool), err_msg=f"{name} step {t}: truncated")
        alive &= ~np.asarray(term, bool)
    eng.close()
    print(f"{name} [{backend}]: free running, {off} of {total} cells beyond {OBS_ATOL}, largest difference {worst:.3g}")
    assert off == 0, f"{name}: {off} of {total} cells differ beyond {OBS_ATOL} (largest difference {worst:.3g})"


@pytest.mark.parametrize("backend", BACKENDS)
def test_crafted_roads_bit_for_bit(backend):
    """lidar_crafted: the float32 pairs of every cell of every hand-placed road are the reference's, bit for bit (the sign of a
    zero velocity included)."""
    g = LidarGolden("lidar_crafted")
    eng = make_engine(backend, g.hwy_config())
    g.load(eng)
    got, want = eng.observe(), g.reference_obs()
    eng.close()
    rng = np.float32(60.0)
    # what the fixture is for (stated on the reference's own values, so that a regenerated fixture cannot lose a case silently)
    assert (want[0, 0, :, 1] != rng).any() and np.all(want[0, 0][want[0, 0, :, 0] != rng][:, 1] == np.float32(30.0 - 25.0))   # later wins
    assert want[1, 0, 0, 1] == np.float32(28.0 - 25.0)                                   # tie of the centre candidates
    assert want[2, 0, 0, 1] == want[3, 0, 0, 1] == np.float32(20.0 - 25.0)               # 1e-9 apart, both orders
    assert want[4, 0, 0, 1] == np.float32(30.0 - 25.0) and want[4, 0, 0, 0] == np.float32(27.5)  # above the rounded value: loses
    assert (want[5] == rng).all() and (want[6, 0, :, 0] != rng).any()                    # the centre decides the range test
    assert want[7, 0, 8, 0] == np.float32(17.5) and want[9, 0, 15, 0] < rng and want[9, 0, 0, 0] == rng  # +-pi and cell 0
    assert want[16, 0, 15, 0] < rng and want[16, 0, 0, 0] == np.float32(1.5) and (want[16, 0, 1:14, 0] == rng).all()
    assert want[10, 0, 4, 0] == np.float32(3.0) and want[10, 0, 12, 0] == np.float32(3.0)  # level with the observer
    assert (want[13, 0, :, 0] < 0).any()                                                 # negative centre distance
    assert (want[15] == rng).all()
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"first differing (road, agent, cell, component): {bad[0]}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", ["lidar_fast", "lidar_ma2", "lidar_n100", "lidar_linear", "lidar_direct"])
def test_rollout_equals_steps(backend, name):
    """hwy_rollout with K = 4 (K x (step launch + lidar launch)) equals four calls of hwy_step, bit for bit: outputs and state."""
    g = LidarGolden(name)
    K = min(g.steps, 4)
    acts = np.stack([g.actions_at(t) for t in range(K)])
    a, b = make_engine(backend, g.hwy_config()), make_engine(backend, g.hwy_config())
    for e in (a, b):
        g.load(e)
    ro = a.rollout(acts)
    steps = [b.step(acts[k]) for k in range(K)]
    assert ro[0].shape == (K, g.E, g.A, *_abi.obs_shape(g.hwy_config()))
    for k in range(K):
        assert np.array_equal(ro[0][k].view(np.uint32), steps[k][0].view(np.uint32)), f"step {k}: obs"
        for j in (1, 2, 3):
            np.testing.assert_array_equal(ro[j][k], steps[k][j], err_msg=f"step {k} output {j}")
    assert not np.array_equal(ro[0][0], ro[0][K - 1])  # (each block holds its own step's observation)
    sa, sb = a.get_state(), b.get_state()
    for key in _abi.STATE_F64 + _abi.STATE_I32:
        np.testing.assert_array_equal(sa[key], sb[key], err_msg=key)
    a.close()
    b.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_autoreset_step_returns_the_new_episodes_lidar(backend):
    """Next-step auto-reset: the step that re-spawns an environment returns the lidar of the NEW episode's first state (reward 0),
    i.e. of the state that step left behind -- checked against the emulated kernel on the engine's own state."""
    from tests.emu import emu
    g = LidarGolden("lidar_crash")
    cfg = g.hwy_config()
    eng = make_engine(backend, cfg)
    g.load(eng)
    eng.set_autoreset(True, base_seed=77, ego_spacing=1.0, vehicles_density=2.0)
    done = np.zeros(g.E, bool)
    respawned = 0
    for t in range(g.steps + 2):
        before = eng.get_state()
        obs, reward, term, trunc, info = eng.step(g.actions_at(t % g.steps))
        st = eng.get_state()
        want = emu.trace(cfg, st)
        assert cells_off(obs, want) == 0, f"step {t}"
        for e in np.flatnonzero(done):
            respawned += 1
            assert st["time"][e] == 0.0 and reward[e, 0] == 0.0 and not term[e]
            assert cells_off(obs[e], emu.trace(cfg, before)[e]) > 0  # not the finished episode's last state
        done = np.asarray(term | trunc, bool)
    eng.close()
    assert respawned >= 3
