"""Device-side traffic management of the intersection scenario (csrc/hwy_ix.h: ix_clear_spawn, ix_spawn_env): the
step kernel clears leaving vehicles, spawns new ones and re-spawns finished episodes on Philox draws.

The random stream is not numpy's; what has to match the reference is the RULE.  The product's host implementation of
that rule (highwayenv_amd/intersection.py: spawn_vehicle / clear_vehicles / make_vehicles_*) is pinned to the
reference's reset(seed=s) and episodes in tests/test_envs_host.py; here it is driven by a fake Generator that hands
out the kernel's own Philox draws in the reference's draw order, and the kernel must produce the same traffic.
"""
import numpy as np
import pytest

from highwayenv_amd import _abi
from highwayenv_amd import intersection as hix
from tests.backends import BACKENDS, make_engine
from tests.spawn_util import philox_uniform2


class PhiloxAsGenerator:
    """The draws one _spawn_vehicle call takes, from the kernel's counters (vehicle id `stream`, 4 x 2 uniforms)."""

    def __init__(self, seed, stream, episode, force_spawn=False):
        u = []
        for d in range(4):
            u.extend(philox_uniform2(int(seed), int(stream), int(episode), d))
        self.u = u
        self.force = force_spawn
        self.k_normal = 0

    def uniform(self, low=None, high=None):
        if low is None:
            return 0.0 if self.force else self.u[0]
        return low + (high - low) * self.u[7]

    def choice(self, rng, size, replace):
        r0 = min(int(self.u[1] * 4), 3)
        r1 = min(int(self.u[2] * 3), 2)
        r1 = r1 + 1 if r1 >= r0 else r1
        return np.array([r0, r1])

    def normal(self, loc=0.0):
        a, b = (self.u[3], self.u[4]) if self.k_normal == 0 else (self.u[5], self.u[6])
        self.k_normal += 1
        return loc + np.sqrt(-2.0 * np.log(1.0 - a)) * np.cos(2 * np.pi * b)


def _config(E, **over):
    cfg = hix.intersection_default_config()
    cfg.update(over)
    return cfg, _abi.make_config(cfg, E, scenario="intersection")


def _assert_same_traffic(got, want, atol=1e-9, what=""):
    pres = (want["flags"] & _abi.F_ABSENT) == 0
    np.testing.assert_array_equal((got["flags"] & _abi.F_ABSENT) == 0, pres, err_msg=f"{what}: present")
    for k in ("lane", "target_lane", "flags", "route"):
        np.testing.assert_array_equal(got[k][pres], want[k][pres], err_msg=f"{what}: {k}")
    for k in ("x", "y", "heading", "speed", "target_speed", "timer", "delta"):
        np.testing.assert_allclose(got[k][pres], want[k][pres], rtol=0, atol=atol, err_msg=f"{what}: {k}")


def _host_reset(backend, cfg, c, seeds, episode):
    """ix_spawn_env restated with the host rule: initial spawns, 45 frames on a host-traffic engine, challenger, ego."""
    E = len(seeds)
    tab = hix.table_from_config(c)
    st = _abi.alloc_state_ix(E, c.num_vehicles)
    n = int(cfg["initial_vehicle_count"])
    for e, sd in enumerate(seeds):
        for t in range(n - 1):
            hix.spawn_vehicle(c, tab, st, e, PhiloxAsGenerator(sd, t, episode), np.linspace(0, 80, n)[t])
    cfg_h = dict(cfg, host_traffic=True)
    eng = make_engine(backend, _abi.make_config(cfg_h, E, scenario="intersection"))
    eng.set_state(st)
    eng.step_frames(None, 3 * int(cfg["simulation_frequency"]))
    st = eng.get_state()
    eng.close()
    for e, sd in enumerate(seeds):
        hix.spawn_vehicle(c, tab, st, e, PhiloxAsGenerator(sd, 500, episode, force_spawn=True), 60, spawn_probability=1.0,
                          go_straight=True, position_deviation=0.1, speed_deviation=0.0)

        class EgoDraw:  # controlled vehicle k draws from stream 501 + k: (its destination,) its position
            k = 0

            def normal(self, loc=0.0, _sd=sd):
                a, b = philox_uniform2(int(_sd), 501 + self.k, int(episode), 0)
                self.k += 1
                return loc + np.sqrt(-2.0 * np.log(1.0 - a)) * np.cos(2 * np.pi * b)

            def integers(self, lo, hi, _sd=sd):  # destination = "o" + str(np_random.integers(1, 4))
                k = min(int(philox_uniform2(int(_sd), 501 + self.k, int(episode), 1)[0] * 3), 2)
                return lo + k

            def uniform(self, *a, **k):  # the challenger already took its draws
                raise AssertionError
        # second half of make_vehicles_after_warmup without its own challenger spawn: replay it with a generator whose
        # first call (the challenger's uniform) rejects the spawn
        class AfterWarmup(EgoDraw):
            def uniform(self, *a, **k):
                return 2.0
        hix.make_vehicles_after_warmup(c, cfg, tab, st, e, AfterWarmup())
    st["time"][...] = 0.0
    return st


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("destination,agents", [("o1", 1), (None, 1), ("o1", 2), (None, 4)])
def test_device_reset_follows_the_reference_rule(backend, destination, agents):
    """agents > 1: MultiAgentIntersectionEnv's loop over ego_id (intersection_env.py:292-318) -- agent k on road o{k % 4},
    the traffic within 20 m of each new controlled vehicle removed, the controlled ones kept."""
    E = 6
    cfg, c = _config(E, max_vehicles=24, destination=destination, controlled_vehicles=agents)
    seeds = np.array([3, 2**40 + 17, 99, 12345678901234567, 0, 7], np.uint64)
    eng = make_engine(backend, c)
    obs = eng.reset(seeds=seeds)
    got = eng.get_state()
    want = _host_reset(backend, cfg, c, seeds, 0)
    _assert_same_traffic(got, want, atol=1e-9, what="reset")
    np.testing.assert_array_equal(got["road_steps"], 45)
    assert (got["time"] == 0).all()
    # the controlled vehicles are the last ones of the list; the first observation row of agent a is its absolute pose
    ctrl = (got["flags"] & _abi.F_CONTROLLED) != 0
    assert (ctrl.sum(1) == agents).all()
    assert obs.shape[:2] == (E, agents)
    cfg_h = dict(cfg, host_traffic=True)
    ref = make_engine(backend, _abi.make_config(cfg_h, E, scenario="intersection"))
    ref.set_state(want)
    np.testing.assert_allclose(obs, ref.observe(), rtol=0, atol=1e-6)
    ref.close()
    eng.close()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("slots", [24, 40])  # 32-thread and 64-thread workgroups (csrc/hwy_ix.h: CAP)
def test_device_step_clears_and_spawns_like_the_host_rule(backend, slots):
    """Same start, same actions: the device-traffic engine after each step == the host-traffic engine + the host
    rule fed with the kernel's Philox draws (stream 1000 + step number)."""
    E = 8
    cfg, c = _config(E, max_vehicles=slots, spawn_probability=0.9, duration=40)
    base = 777
    dev = make_engine(backend, c)
    dev.reset(seeds=np.uint64(base) + np.arange(E, dtype=np.uint64))
    dev.set_autoreset(False, base_seed=base)
    cfg_h = dict(cfg, host_traffic=True)
    ch = _abi.make_config(cfg_h, E, scenario="intersection")
    host = make_engine(backend, ch)
    host.set_state(dev.get_state())
    tab = hix.table_from_config(c)
    rng = np.random.default_rng(0)
    n_spawn = n_clear = 0
    for t in range(22):
        acts = rng.integers(0, 3, size=(E, 1)).astype(np.int32)
        o1, r1, te1, tr1, _ = dev.step(acts)
        o2, r2, te2, tr2, _ = host.step(acts)
        np.testing.assert_array_equal(o1, o2)
        np.testing.assert_array_equal(r1, r2)
        np.testing.assert_array_equal(te1, te2)
        st = host.get_state()
        before = ((st["flags"] & _abi.F_ABSENT) == 0).sum(1)
        for e in range(E):
            hix.clear_vehicles(ch, tab, st, e)
        mid = ((st["flags"] & _abi.F_ABSENT) == 0).sum(1)
        for e in range(E):
            hix.spawn_vehicle(ch, tab, st, e, PhiloxAsGenerator(base + e, 1000 + t, 0), spawn_probability=0.9)
        after = ((st["flags"] & _abi.F_ABSENT) == 0).sum(1)
        n_clear += int((before - mid).sum())
        n_spawn += int((after - mid).sum())
        _assert_same_traffic(dev.get_state(), st, atol=1e-12, what=f"step {t}")
        host.set_state(st)
    assert n_spawn > 10 and n_clear > 3
    dev.close()
    host.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_autoreset_next_step_semantics(backend):
    E = 6
    cfg, c = _config(E, max_vehicles=24, duration=4)
    base = 4242
    eng = make_engine(backend, c)
    eng.reset(seeds=np.uint64(base) + np.arange(E, dtype=np.uint64))
    eng.set_autoreset(True, base_seed=base)
    done_prev = np.zeros(E, bool)
    episode = np.zeros(E, int)
    n_resets = 0
    for t in range(11):
        obs, reward, term, trunc, info = eng.step(np.ones((E, 1), np.int32))
        st = eng.get_state()
        for e in np.nonzero(done_prev)[0]:
            episode[e] += 1
            want = _host_reset(backend, cfg, c, [base + e], int(episode[e]))
            _assert_same_traffic({k: v[e:e + 1] for k, v in st.items() if v.ndim == 2},
                                 {k: v for k, v in want.items() if v.ndim == 2}, atol=1e-9, what=f"step {t} env {e}")
            assert reward[e, 0] == 0 and not term[e] and not trunc[e] and st["time"][e] == 0
            n_resets += 1
        done_prev = term | trunc
    assert n_resets >= E  # duration 4: every env was truncated (or terminated) and re-spawned
    eng.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_when_the_next_episode_is_prepared_cannot_change_any_result(backend):
    """hwy_config.tune_ix_no_prewarm / tune_ix_prewarm_frames only move the warm-up frames of an environment's NEXT episode
    between launches (inline at the auto-reset, 15 frames per launch, the default third of a step, 2 frames): the episodes --
    two controlled vehicles, random destinations -- must be the same BIT FOR BIT."""
    E = 6
    rng = np.random.default_rng(11)
    acts = rng.integers(0, 3, size=(9, E, 2)).astype(np.int32)
    runs = []
    for tuning in ({"ix_no_prewarm": 1}, {"ix_prewarm_frames": 15}, None, {"ix_prewarm_frames": 2}):
        cfg = hix.intersection_default_config()
        cfg.update(max_vehicles=24, duration=3, controlled_vehicles=2, destination=None)
        eng = make_engine(backend, _abi.make_config(cfg, E, scenario="intersection", tuning=tuning))
        eng.reset(seeds=np.uint64(77) + np.arange(E, dtype=np.uint64))
        eng.set_autoreset(True, base_seed=77)
        rows = []
        for t in range(acts.shape[0]):
            out = eng.step(acts[t])
            st = eng.get_state()
            pres = (st["flags"] & _abi.F_ABSENT) == 0
            rows.append((out[0].copy(), out[1].copy(), out[2].copy(), out[3].copy(),
                         {k: np.where(pres, v, 0) for k, v in st.items() if v.ndim == 2}))
        runs.append(rows)
        eng.close()
    n_done = 0
    for other in runs[1:]:
        for (o0, r0, t0, u0, s0), (o1, r1, t1, u1, s1) in zip(runs[0], other):
            np.testing.assert_array_equal(o0, o1)
            np.testing.assert_array_equal(r0, r1)
            np.testing.assert_array_equal(t0, t1)
            np.testing.assert_array_equal(u0, u1)
            for k in s0:
                np.testing.assert_array_equal(s0[k], s1[k], err_msg=k)
            n_done += int((t0 | u0).sum())
    assert n_done >= 3 * E  # every variant went through auto-resets


@pytest.mark.gpu
def test_spawn_counters_report_what_the_slot_cap_drops():
    """The reference's vehicle list is unbounded (intersection_env.py:324-352); the engine has ``max_vehicles`` slots and
    drops a spawn that finds them all taken.  hwy_get_counters makes that deviation measurable: with 6 slots drops
    happen, with BASELINE config 4's 30 slots the printed rate is what DESIGN.md quotes; spawns + drops = attempts."""
    from highwayenv_amd.engine import Engine
    rates = {}
    for cap in (6, 30, 48):
        cfg_d, cfg = _config(512, max_vehicles=cap, observation={"type": "OccupancyGrid"})
        eng = Engine(cfg)
        eng.reset(base_seed=3)
        eng.set_autoreset(True, base_seed=4)
        c0 = eng.counters(reset=True)
        assert c0["ix_spawns"] > 0  # the initial traffic of 512 episodes
        rng = np.random.default_rng(0)
        present_before = ((eng.get_state()["flags"] & _abi.F_ABSENT) == 0).sum()
        for t in range(40):
            eng.step(rng.integers(0, 3, size=(512, 1)))
        c = eng.counters()
        assert eng.counters(reset=True) == c and eng.counters() == {"ix_spawns": 0, "ix_spawns_dropped": 0, "nonfinite_stores": 0}
        attempts = c["ix_spawns"] + c["ix_spawns_dropped"]
        assert attempts > 512  # spawn_probability 0.6 per env-step, minus the ones too close to somebody
        rates[cap] = c["ix_spawns_dropped"] / attempts
        eng.close()
    print(f"\nintersection-v0 spawn drop rate by slot capacity: " + ", ".join(f"{k} slots: {100 * v:.3f} %" for k, v in rates.items()))
    assert rates[6] > 0.05 and rates[48] == 0.0 and rates[30] <= rates[6]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("agents,slots", [(1, 4), (3, 5), (4, 4)])
def test_a_controlled_vehicle_is_never_the_dropped_spawn(backend, agents, slots):
    """With fewer slots than the initial traffic fills, the device reset must still create EVERY controlled vehicle (it
    replaces the most recent traffic vehicle; the reference's list is unbounded, intersection_env.py:302-311) -- otherwise
    the agent's observation / reward rows would be unwritten and an episode without an ego would never terminate."""
    E = 6 if backend == "emu" else 64
    over = {"max_vehicles": slots, "initial_vehicle_count": 12, "controlled_vehicles": agents, "spawn_probability": 1.0}
    if agents > 1:
        d = hix.intersection_default_config()
        over.update({"action": {"type": "MultiAgentAction", "action_config": d["action"]},
                     "observation": {"type": "MultiAgentObservation", "observation_config": d["observation"]}})
    cfg_d, cfg = _config(E, **over)
    eng = make_engine(backend, cfg)
    eng.reset(base_seed=17)
    eng.set_autoreset(True, base_seed=18)
    for t in range(4):
        st = eng.get_state()
        pres = (st["flags"] & _abi.F_ABSENT) == 0
        ctrl = pres & ((st["flags"] & _abi.F_CONTROLLED) != 0)
        assert ctrl.sum(1).tolist() == [agents] * E, f"step {t}: controlled vehicles per env"
        assert (pres.sum(1) <= slots).all() and (pres == (np.arange(slots)[None, :] < pres.sum(1)[:, None])).all()
        obs, reward, term, trunc, info = eng.step(np.ones((E, agents), np.int32))
        assert np.isfinite(obs).all() and np.isfinite(reward).all()
    eng.close()
