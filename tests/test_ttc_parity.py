"""The time-to-collision grid and the finite-MDP planner (csrc/hwy_ttc.h: hwy_ttc_kernel, launched on the engine's stream) against
the unmodified reference's fixtures (tests/golden/ttc), on the CPU emulation of the kernel source (``emu``) and on the MI355X
(``hip``).

The yardsticks are the reference's own ``compute_ttc_grid`` and the tables of its ``to_finite_mdp()``, recorded at reset and after
every step of a run and on the hand-placed roads of ``ttc_crafted``.  Grids are compared array-equal (the fixtures hold no candidate
within 1e-9 of a cell boundary: the generator asserts it), ``transition`` / ``terminal`` / ``state`` exactly and ``reward`` bit for
bit.  The planner's Q row and action are compared with ``==`` to a numpy fixed-point iteration on the reference's recorded tables.

On the engine's own states (GPU only) the device is held to the emulation bit for bit and to a numpy restatement of the grid
(tests/ttc_util.py: restate_grid); a differing cell is accepted only where the restatement finds a candidate within 1e-9 of a
cell boundary feeding it, in at most 1 grid of 1000 -- and in none when every heading is 0.

The device-pointer entry points (``hwy_ttc_grid_device`` / ``hwy_mdp_plan_device``, every combination of their optional outputs, into
torch tensors on the engine's stream) are held to the host-pointer forms bit for bit, and the host-pointer forms' own buffer to a
grid that grows between calls (GPU only)."""
import functools

import numpy as np
import pytest

from highwayenv_amd import _abi, finite_mdp
from tests.ttc_util import BACKENDS, FIXTURES, TtcGolden, fixed_point, make_engine, restate_grid

GAMMAS = [1.0, 0.8]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_grids(backend, name):
    """Every recorded state loaded: the grid of every controlled vehicle is the reference's, array-equal -- from the grid entry
    point and from the planner's optional grid output alike."""
    g = TtcGolden(name)
    eng = make_engine(backend, g.hwy_config())
    params = g.params()
    for index in g.indices():
        g.load(eng, index)
        want = g.get("grid", index)
        got = eng.ttc_grid(params)
        assert got.dtype == np.float32 and got.shape == want.shape
        np.testing.assert_array_equal(got.astype(np.float64), want, err_msg=f"{name} state {index}")
        _, _, planned_on = eng.mdp_plan(params, return_grid=True)
        np.testing.assert_array_equal(planned_on, got, err_msg=f"{name} state {index}: the planner's grid")
    eng.close()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", [n for n in FIXTURES if TtcGolden(n).has_tables])
def test_fixture_tables(backend, name):
    """The tables the host builds on the device's grid (highwayenv_amd/finite_mdp.py) are the ones the reference hands to
    DeterministicMDP: transition, terminal and state exactly, reward bit for bit."""
    g = TtcGolden(name)
    cfg = g.hwy_config()
    eng = make_engine(backend, cfg)
    params = g.params()
    for index in g.indices():
        g.load(eng, index)
        grid = eng.ttc_grid(params).astype(np.float64)
        st = eng.get_state()
        for e in range(g.E):
            i = cfg.agent_index[0]
            mdp = finite_mdp.build(grid[e, 0], int(st["speed_index"][e, i]), int(st["lane"][e, i]), g.config)
            what = f"{name} state {index} env {e}"
            np.testing.assert_array_equal(mdp.transition, g.get("transition", index)[e], err_msg=what)
            np.testing.assert_array_equal(mdp.terminal, g.get("terminal", index)[e], err_msg=what)
            assert mdp.state == int(g.get("state", index)[e]) and mdp.original_shape == grid.shape[2:], what
            assert mdp.reward.dtype == np.float64
            np.testing.assert_array_equal(_bits(mdp.reward), _bits(g.get("reward", index)[e]), err_msg=what + ": reward bits")
    eng.close()


@functools.lru_cache(maxsize=None)
def _reference_solution(name: str, gamma: float):
    """{index: (Q rows [E, A, 5], actions [E, A])} of the numpy fixed-point iteration on the reference's recorded tables (computed
    once, shared by the backends).  Two-agent fixtures hold no tables (the reference's to_finite_mdp() cannot run under
    MultiAgentAction): theirs are built from the reference's recorded GRID of each agent by highwayenv_amd/finite_mdp.py, which
    test_fixture_tables holds to the reference on every single-agent fixture."""
    g = TtcGolden(name)
    cfg = g.hwy_config()
    T = g.params().time_steps
    out = {}
    for index in g.indices():
        st = g.state("init" if index is None else "step", index)
        q, act = np.zeros((g.E, g.A, 5)), np.zeros((g.E, g.A), np.int32)
        for e in range(g.E):
            for a in range(g.A):
                i = cfg.agent_index[a]
                if g.has_tables:
                    tr, rw, te, s = (g.get(k, index)[e] for k in ("transition", "reward", "terminal", "state"))
                else:
                    m = finite_mdp.build(g.get("grid", index)[e, a], int(st["speed_index"][e, i]), int(st["lane"][e, i]), g.config)
                    tr, rw, te, s = m.transition, m.reward, m.terminal, m.state
                _, table = fixed_point(tr, rw, te.astype(bool), gamma, T + 1)
                q[e, a], act[e, a] = table[int(s)], int(np.argmax(table[int(s)]))
        out[index] = (q, act)
    return out


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("name", FIXTURES)
def test_planner_equals_numpy_fixed_point(backend, name, gamma):
    """Q(state, .) and the action of the one backward sweep equal the fixed point of
    V <- max_a(reward + gamma * where(terminal, 0, V[transition])) iterated in numpy (T + 1 sweeps from zeros; one more changes
    nothing), compared with ``==``."""
    g = TtcGolden(name)
    want = _reference_solution(name, gamma)
    eng = make_engine(backend, g.hwy_config())
    params = g.params(gamma)
    for index in g.indices():
        g.load(eng, index)
        action, q, _ = eng.mdp_plan(params, return_q=True)
        assert np.array_equal(q, want[index][0]), f"{name} state {index} gamma {gamma}: Q\n{q}\n{want[index][0]}"
        assert np.array_equal(action, want[index][1]), f"{name} state {index} gamma {gamma}: action"
        only_action, none_q, _ = eng.mdp_plan(params)
        assert none_q is None and np.array_equal(only_action, action)
    eng.close()


def test_crafted_roads_are_what_they_are_for():
    """Stated on the reference's own grids, so that a regenerated fixture cannot lose a case silently."""
    g = TtcGolden("ttc_crafted")
    w = g.get("grid")[:, 0]                                   # [road, V, L, T]
    assert not w[0, 1].any() and w[0, 2, 1, 6] == 1.0          # other.speed == the target speed 25: that ego speed skips it
    assert w[1, 1, 1, 5] == 0.5 and w[1, 1, 2, 4] == 0.5 and not (w[1, 1] == 1.0).any()  # not_zero's +-0.01: margin points only
    assert w[2, 0, 1, 3] == 1.0 and not w[2, 2].any()          # a faster vehicle behind hits the slow ego only
    assert w[3, 1, 1, 4] == 1.0 and w[3, 1, 3, 8] == 1.0       # oncoming
    assert (w[4, 1, 1] == [0, 0, 0, .5, 1, .5, 0, 0, 0, 0]).all() and (w[4, 0, 1, 7:] == [.5, 1, .5]).all()  # exact multiples: ONE cell
    assert (w[5, 1, 2] == [0] * 9 + [.5]).all()                # ttc / tq == T is out of range, the rear margin (9.5) is in
    assert w[6].any() and w[8].any() and not w[9].any()
    assert w[7, 0, 2, 0] == 1.0 and w[7, 2, 2, 0] == 1.0       # distance 0: time 0 whatever the closing speed
    assert np.abs(g.z["init_heading"][6]).max() == 0.3 and g.z["init_heading"][8, 0] == 0.2
    # the same equality within reach of not_zero(0) = 0.01: 0.037 / 0.01 = 3.7 s would mark cells 3 and 4 of ego speed 25
    assert not w[10, 1].any() and w[10, 2, 2, 0] == 1.0 and w[10, 0, 2, 0] == 0.5


# ---- the engine's own states (GPU) --------------------------------------------------------------------------------------------------
STEPS = 30


@functools.lru_cache(maxsize=None)
def _engine_run(n_vehicles: int):
    """E = 8 environments of highway-fast-v0 with `n_vehicles` vehicles on the MI355X, 30 steps of random actions with auto-reset:
    after reset and after every step the state, the device's grid and plan (gamma 0.8) -- recorded once, shared by the tests."""
    from highwayenv_amd.engine import Engine
    d = _abi.highway_fast_default_config()
    d.update({"vehicles_count": n_vehicles - 1, "lanes_count": 4, "duration": 12, "vehicles_density": 1.5})
    cfg = _abi.make_config(d, 8, fast=True)
    params = _abi.ttc_params(d, gamma=0.8)
    eng = Engine(cfg)
    eng.reset(seeds=np.arange(8, dtype=np.uint64) + 100, ego_spacing=d["ego_spacing"], vehicles_density=d["vehicles_density"])
    eng.set_autoreset(True, base_seed=7, ego_spacing=d["ego_spacing"], vehicles_density=d["vehicles_density"])
    rng = np.random.default_rng(n_vehicles)
    record = []
    for t in range(STEPS + 1):
        if t:
            eng.step(rng.integers(0, 5, size=(8, 1)).astype(np.int32))
        action, q, grid = eng.mdp_plan(params, return_q=True, return_grid=True)
        record.append((eng.get_state(), grid, action, q, eng.ttc_grid(params)))
    eng.close()
    return cfg, params, record


@pytest.mark.gpu
@pytest.mark.parametrize("n_vehicles", [20, 130])
def test_hip_equals_emulation_on_engine_states(n_vehicles):
    """The MI355X against the CPU emulation of the same kernel source on the states the engine itself produced: grid, Q and action
    bit for bit."""
    from tests.emu import emu
    cfg, params, record = _engine_run(n_vehicles)
    episodes = 0
    for t, (st, grid, action, q, grid_alone) in enumerate(record):
        e_action, e_q, e_grid = emu.mdp_plan(cfg, st, params, return_q=True, return_grid=True)
        np.testing.assert_array_equal(grid, e_grid, err_msg=f"N={n_vehicles} step {t}: grid")
        np.testing.assert_array_equal(grid_alone, e_grid, err_msg=f"N={n_vehicles} step {t}: grid entry point")
        np.testing.assert_array_equal(_bits(q), _bits(e_q), err_msg=f"N={n_vehicles} step {t}: Q")
        np.testing.assert_array_equal(action, e_action, err_msg=f"N={n_vehicles} step {t}: action")
        episodes += int((st["time"] == 0).sum())
    assert episodes > 8  # (auto-reset re-spawned environments during the run)
    assert len({tuple(r[2].ravel()) for r in record}) > 1 and any(r[1].any() for r in record)


@pytest.mark.gpu
@pytest.mark.parametrize("n_vehicles", [20, 130])
def test_hip_against_numpy_restatement(n_vehicles):
    """The device's grids against the numpy restatement on the same states.  A differing cell is accepted only where the restatement
    finds a candidate within 1e-9 of a cell boundary feeding it; at most 1 grid in 1000 may be excused that way."""
    cfg, params, record = _engine_run(n_vehicles)
    grids = excused = 0
    for t, (st, grid, _, _, _) in enumerate(record):
        want, edge, _, _ = restate_grid(cfg, st, params)
        differ = grid.astype(np.float64) != want
        assert not (differ & ~edge).any(), f"N={n_vehicles} step {t}: {np.argwhere(differ & ~edge)[:4]} differ away from any cell boundary"
        excused += int(differ.any(axis=(2, 3, 4)).sum())
        grids += grid.shape[0] * grid.shape[1]
    print(f"N={n_vehicles}: {excused} of {grids} grids excused by a candidate within 1e-9 of a cell boundary")
    assert excused * 1000 <= grids


@pytest.mark.gpu
def test_hip_against_numpy_restatement_headings_zero():
    """With every heading exactly 0 the arithmetic is the restatement's own: no cell differs, none is excused."""
    from highwayenv_amd.engine import Engine
    cfg, params, record = _engine_run(20)
    eng = Engine(cfg)
    for st, *_ in record[::6]:
        st = {k: v.copy() for k, v in st.items()}
        st["heading"][...] = 0.0
        eng.set_state(st)
        want, _, _, _ = restate_grid(cfg, st, params)
        np.testing.assert_array_equal(eng.ttc_grid(params).astype(np.float64), want)
    eng.close()


def _device_case(case: str):
    """(cfg, params, states): ``ttc_ma2`` -- two agents, the small capacity class; ``ttc_max`` -- 8192 cells, 128 states; ``fuzz4`` --
    case 4 of tests/test_ttc_fuzz.py: four agents on 7 x 16 x 64 cells, 128 slots."""
    if case == "fuzz4":
        from tests.test_ttc_fuzz import _case
        _, cfg, params, rows, _, _ = _case(4)
        return cfg, params, [rows[0][0], rows[1][0]]
    g = TtcGolden(case)
    return g.hwy_config(), g.params(0.8), [g.state("init"), g.state("step", g.steps - 1)]


GUARD = 64  # elements behind every device output that must stay as they were


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["ttc_ma2", "ttc_max", "fuzz4"])
def test_device_entry_points_equal_the_host_pointer_forms(case):
    """hwy_ttc_grid_device and hwy_mdp_plan_device with d_q / d_grid given or null, into torch tensors on the engine's stream: row
    r = e * A + a writes grid + r * cells, action + r and q + r * 5 -- bit for bit what hwy_ttc_grid / hwy_mdp_plan copy to the
    host for the same state -- an output that is not asked for is not written, and nothing is written behind an output's end."""
    import itertools

    import torch

    from highwayenv_amd.engine import Engine
    cfg, params, states = _device_case(case)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    eng = Engine(cfg, device=0, stream=stream.cuda_stream)
    rows, cells = cfg.num_envs * cfg.num_agents, int(np.prod(eng.ttc_shape(params)))
    assert rows > cfg.num_envs or case == "ttc_max"
    with torch.cuda.stream(stream):
        for k, st in enumerate(states):
            eng.set_state(st)
            want_grid = eng.ttc_grid(params).reshape(rows, cells)
            want_action, want_q, _ = eng.mdp_plan(params, return_q=True)
            assert want_grid.any() and not np.isnan(want_q).any()
            for with_q, with_grid in [(None, True)] + list(itertools.product((True, False), (True, False))):
                grid = torch.full((rows * cells + GUARD,), -3.0, dtype=torch.float32, device=dev)
                action = torch.full((rows + GUARD,), -7, dtype=torch.int32, device=dev)
                q = torch.full((rows * 5 + GUARD,), -9.0, dtype=torch.float64, device=dev)
                if with_q is None:
                    eng.ttc_grid_device(params, grid.data_ptr())
                else:
                    eng.mdp_plan_device(params, action.data_ptr(), q.data_ptr() if with_q else 0, grid.data_ptr() if with_grid else 0)
                stream.synchronize()
                what = f"{case} state {k}: " + ("ttc_grid_device" if with_q is None else f"mdp_plan_device(q={with_q}, grid={with_grid})")
                grid, action, q = grid.cpu().numpy(), action.cpu().numpy(), q.cpu().numpy()
                if with_grid:
                    np.testing.assert_array_equal(grid[:rows * cells].reshape(rows, cells), want_grid, err_msg=what + ": grid")
                else:
                    assert (grid == -3.0).all(), what + ": a grid was written that was not asked for"
                if with_q:
                    np.testing.assert_array_equal(_bits(q[:rows * 5]), _bits(want_q.reshape(-1)), err_msg=what + ": Q bits")
                else:
                    assert (q == -9.0).all(), what + ": Q was written that was not asked for"
                if with_q is None:
                    assert (action == -7).all(), what
                else:
                    np.testing.assert_array_equal(action[:rows], want_action.reshape(-1), err_msg=what + ": action")
                assert (grid[rows * cells:] == -3.0).all() and (action[rows:] == -7).all() and (q[rows * 5:] == -9.0).all(), \
                    what + ": written behind the end of an output"
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("first", ["ttc_grid", "mdp_plan"])
def test_host_pointer_buffer_grows_between_calls(first):
    """One engine with 8 speeds and 16 lanes, T = 1 (128 cells), then T = 64 (8192 cells: the engine frees its grid buffer and
    allocates a larger one), then T = 10 (the larger buffer stays): every result equals the emulation's for the same state and
    params, whichever of the two host-pointer entry points meets the growing grid first."""
    from highwayenv_amd.engine import Engine
    from tests.emu import emu
    g = TtcGolden("ttc_max")
    cfg, st = g.hwy_config(), g.state("init")
    eng = Engine(cfg)
    eng.set_state(st)
    for horizon, tq in ((1.0, 1.0), (6.4, 0.1), (10.0, 1.0)):
        params = _abi.ttc_params(g.config, horizon=horizon, time_quantization=tq, gamma=0.8)
        e_action, e_q, e_grid = emu.mdp_plan(cfg, st, params, return_q=True, return_grid=True)
        assert e_grid.shape[2:] == (8, 16, params.time_steps) and e_grid.any()
        got = {}
        for call in (("ttc_grid", "mdp_plan") if first == "ttc_grid" else ("mdp_plan", "ttc_grid")):
            got[call] = eng.ttc_grid(params) if call == "ttc_grid" else eng.mdp_plan(params, return_q=True, return_grid=True)
        what = f"T = {params.time_steps}"
        np.testing.assert_array_equal(got["ttc_grid"], e_grid, err_msg=what + ": grid entry point")
        action, q, grid = got["mdp_plan"]
        np.testing.assert_array_equal(grid, e_grid, err_msg=what + ": the planner's grid")
        np.testing.assert_array_equal(_bits(q), _bits(e_q), err_msg=what + ": Q bits")
        np.testing.assert_array_equal(action, e_action, err_msg=what + ": action")
    eng.close()


@pytest.mark.gpu
def test_vector_env_torch_plan_loop_equals_numpy_front_end():
    """HighwayVectorEnv(output="torch"): 20 iterations of step(plan()) -- the plan an int32 device tensor, the step fed by it without
    a host copy -- give the actions, observations and rewards of the same loop through the numpy front end."""
    import torch

    from highwayenv_amd.vector import HighwayVectorEnv
    config = {"vehicles_count": 20, "duration": 8}
    dev_env = HighwayVectorEnv("highway-fast-v0", 8, config=config, output="torch")
    np_env = HighwayVectorEnv("highway-fast-v0", 8, config=config, output="numpy")
    obs_d, _ = dev_env.reset(seed=3)
    obs_n, _ = np_env.reset(seed=3)
    np.testing.assert_array_equal(obs_d.cpu().numpy(), obs_n)
    seen = set()
    for t in range(20):
        plan_d, plan_n = dev_env.plan(gamma=0.9), np_env.plan(gamma=0.9)
        assert isinstance(plan_d, torch.Tensor) and plan_d.is_cuda and plan_d.dtype == torch.int32 and plan_d.shape == (8,)
        a = plan_d.cpu().numpy()
        np.testing.assert_array_equal(a, plan_n, err_msg=f"iteration {t}: actions")
        seen.update(a.tolist())
        obs_d, rew_d, term_d, trunc_d, _ = dev_env.step(plan_d)
        obs_n, rew_n, term_n, trunc_n, _ = np_env.step(plan_n)
        np.testing.assert_array_equal(obs_d.cpu().numpy(), obs_n, err_msg=f"iteration {t}: observations")
        np.testing.assert_array_equal(rew_d.cpu().numpy(), rew_n, err_msg=f"iteration {t}: rewards")
        np.testing.assert_array_equal(term_d.cpu().numpy(), term_n)
        np.testing.assert_array_equal(trunc_d.cpu().numpy(), trunc_n)
    assert len(seen) > 1
    dev_env.close()
    np_env.close()
