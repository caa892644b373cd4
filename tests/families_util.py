"""Shared helpers of the oracle comparisons of the three straight-road families beside IDM with meta-actions -- the Linear traffic
family, direct ego control (``DiscreteAction``) and the ``LidarObservation`` -- : one ``make_engine`` over the four emulator
drivers and the HIP engine, the hand-over of what an engine keeps beside its state planes (behaviour parameters, stored controls)
to the engine and to the oracle, and ``rollout``, the free-running comparison every edge-case and fuzz test of the straight road
goes through (tests/test_edge_cases.py re-exports it)."""
from __future__ import annotations

import numpy as np

from highwayenv_amd import _abi, spawn
from oracle import oracle
from tests.backends import make_engine  # noqa: F401  (re-exported)
from tests.golden_util import assert_obs_close, assert_state_close
from tests.lidar_util import cells_off


def load_engine(eng, st: dict) -> None:
    """A state dict with its extras (``behavior``; ``ctl_accel`` / ``ctl_steer``) onto an engine."""
    eng.set_state(st)
    if eng.cfg.traffic_model == _abi.TRAFFIC_LINEAR:
        eng.set_behavior(st["behavior"])
    if eng.cfg.ego_control == _abi.EGO_DIRECT:
        eng.set_controls(st["ctl_accel"], st["ctl_steer"])


def engine_state(eng) -> dict:
    """The engine's state planes plus its extras, as the oracle takes them."""
    st = eng.get_state()
    if eng.cfg.traffic_model == _abi.TRAFFIC_LINEAR:
        st["behavior"] = np.ascontiguousarray(eng.get_behavior())
    if eng.cfg.ego_control == _abi.EGO_DIRECT:
        a, s = eng.get_controls()
        st["ctl_accel"], st["ctl_steer"] = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(s, np.float64)
    return st


def golden_state(g, prefix: str = "init", index=None, envs=None) -> dict:
    """A recorded state of a fixture of tests/golden/traffic, control or lidar with the extras the oracle needs: the drawn
    parameters (``init_behavior``) and the agents' stored action (``*_act_accel`` / ``*_act_steering``)."""
    st = g.state(prefix, index, envs=envs)
    cfg = g.hwy_config()
    rows = slice(None) if envs is None else envs
    if cfg.traffic_model == _abi.TRAFFIC_LINEAR:
        st["behavior"] = np.ascontiguousarray(g.z["init_behavior"][rows], np.float64)
    if cfg.ego_control == _abi.EGO_DIRECT:
        agents = list(cfg.agent_index[:cfg.num_agents])
        for key, plane in (("ctl_accel", "act_accel"), ("ctl_steer", "act_steering")):
            a = g.z[f"{prefix}_{plane}"]
            a = a if index is None else a[index]
            st[key] = np.ascontiguousarray(a[rows][:, agents], np.float64)
    return st


def check_free_running_steps(g):
    """A recorded run of the reference (a fixture of tests/golden/traffic, control or lidar, or a live run in the same layout)
    through the ORACLE, free running from the reference's initial state: observations 1e-6 (Lidar: no cell beyond it), reward and
    speed 1e-9, terminated / truncated / crashed exact, the state after every step at 1e-8 with lanes, target lanes and flags exact;
    a direct-control ego's speed and stored acceleration bit for bit (exactly rounded operations, tests/test_control_parity.py);
    each environment up to and including its first terminated step.  Returns (Lidar cells compared, largest Lidar difference)."""
    cfg = g.hwy_config()
    lidar = cfg.obs_type == _abi.OBS_LIDAR
    agents = list(cfg.agent_index[:cfg.num_agents])
    st = golden_state(g)
    z = g.z
    obs0 = oracle.observe(cfg, st)
    cells, worst = 0, 0.0

    def compare_obs(got, want, what):
        nonlocal cells, worst
        want = np.asarray(want).reshape(got.shape)
        if lidar:  # no cell beyond 1e-6: none is exempt
            assert cells_off(got, want) == 0, f"{what}: {cells_off(got, want)} lidar cells beyond 1e-6"
            cells += got[..., 0].size
            worst = max(worst, float(np.abs(got.astype(np.float64) - want).max(initial=0)))
        else:
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-6, err_msg=what)

    compare_obs(obs0, z["obs0"], f"{g.name} reset")
    alive = np.ones(g.E, bool)
    for t in range(g.steps):
        obs, reward, term, trunc, info = oracle.step(cfg, st, g.actions_at(t))
        what = f"{g.name} step {t}"
        rows = np.flatnonzero(alive)
        compare_obs(obs[rows], z["obs"][t].reshape(obs.shape)[rows], what)
        np.testing.assert_allclose(reward[rows, 0], z["reward"][t][rows], rtol=0, atol=1e-9, err_msg=what)
        np.testing.assert_array_equal(term[rows], z["terminated"][t][rows].astype(bool), err_msg=what)
        np.testing.assert_array_equal(trunc[rows], z["truncated"][t][rows].astype(bool), err_msg=what)
        np.testing.assert_allclose(info["speed"][rows], z["step_speed"][t][rows][:, agents], rtol=0, atol=1e-9, err_msg=what)
        np.testing.assert_array_equal(info["crashed"][rows], z["step_crashed"][t][rows][:, agents] != 0, err_msg=what)
        want = golden_state(g, "step", t)
        assert_state_close({k: st[k][rows] for k in want}, {k: v[rows] for k, v in want.items()}, atol=1e-8, what=what)
        if cfg.ego_control == _abi.EGO_DIRECT:
            for k in ("ctl_accel", "ctl_steer"):
                np.testing.assert_array_equal(st[k][rows], want[k][rows], err_msg=f"{what}: {k}")
            np.testing.assert_array_equal(st["speed"][rows][:, agents], want["speed"][rows][:, agents], err_msg=f"{what}: the egos' speed")
        alive &= ~term
    return cells, worst


def assert_lidar_of_own_state(cfg, eng, obs, what: str, rows=None) -> None:
    """The Lidar observation a step returned against the oracle's trace of the state THAT STEP LEFT on the engine: the same
    positions go into both, so only the <= 2 ulp between the kernel's atan2 / sincos and libm separate them -- no cell beyond 1e-6,
    no exclusions."""
    want = oracle.observe(cfg, eng.get_state())
    rows = slice(None) if rows is None else rows
    off = cells_off(obs[rows], want[rows])
    assert off == 0, (f"{what}: {off} lidar cells beyond 1e-6 of the oracle's trace of the engine's own state "
                      f"(largest difference {np.nanmax(np.abs(obs[rows].astype(np.float64) - want[rows])):.3g})")


def comparable(ref, margin, live, compare_wrecks=False):
    """(wreck, ok) [E] after an oracle step on `ref`: which environments hold a wreck, and which live ones are compared in full.
    The step of an env's first collision is compared like any other (terminal observation, reward, positions) unless a push
    direction sits on the knife edge (|d.normal| < 1e-9, utils.py:232-236); assert_state_close compares |impact|
    (free-running: the engine's state may differ from the oracle's by the 1e-7 the previous steps are held to, so a push
    direction decided by |d.normal| below 1e-6 can flip -- two cars tracking one lane centre are that close laterally).
    `margin` [E]: oracle.impact_margins(...).margin.min(1) of that step."""
    wreck = ((ref["flags"] & (_abi.F_CRASHED | _abi.F_HAS_IMPACT)) != 0).any(1)
    return wreck, live & (~wreck | compare_wrecks | (margin >= 1e-6))


def compare_step(cfg, eng, outputs, ref, ref_outputs, wreck, ok, live, what, trunc_rows=slice(None)):
    """One policy step of an engine (`outputs` of eng.step) against the same step of the oracle (`ref` after it, `ref_outputs`):
    terminated exact on `live`, truncated exact on `trunc_rows`, reward 1e-9 on `ok`; state -- and the stored controls of a
    direct-control ego -- and observation at 1e-7 / 1e-6 on wreck-free `ok` rows, 2.5e-6 / 5e-6 on the step of a collision; a Lidar
    observation against the oracle's trace of the engine's own state instead, on every environment.  Returns the engine's state."""
    obs, reward, term, trunc = outputs[:4]
    o2, r2, te2, tr2 = ref_outputs[:4]
    direct, lidar = cfg.ego_control == _abi.EGO_DIRECT, cfg.obs_type == _abi.OBS_LIDAR
    np.testing.assert_array_equal(term[live], te2[live], err_msg=what)
    np.testing.assert_array_equal(trunc[trunc_rows], tr2[trunc_rows], err_msg=what)
    np.testing.assert_allclose(reward[ok], r2[ok], rtol=0, atol=1e-9, err_msg=what)
    got = eng.get_state()
    if lidar:
        assert_lidar_of_own_state(cfg, eng, obs, what)
    # free-running (no re-synchronisation of live environments): every step without a collision at 1e-7; the step of a
    # collision at 2.5e-6 -- the minimum-translation vector is a difference of projected corner coordinates, i.e. it carries
    # the two bodies' heading differences times a 2.7 m lever arm on top of their position differences (largest seen in 20 000
    # random configurations: 1.2e-6 m); un-normalised relative features are differences of two such positions
    for rows, atol, atol_obs in ((ok & ~wreck, 1e-7, 1e-6), (ok & wreck, 2.5e-6, 5e-6)):
        if not lidar:
            assert_obs_close(obs[rows], o2[rows], bool(cfg.flags & _abi.C_GRID_IMAGE), what, atol=atol_obs)
        assert_state_close({k: v[rows] for k, v in got.items()}, {k: ref[k][rows] for k in got}, atol=atol, what=what)
        if direct:  # the stored action: a table entry, or what clip_actions made of it (bound - speed, -1.0 * speed)
            for a, key in zip(eng.get_controls(), ("ctl_accel", "ctl_steer")):
                np.testing.assert_allclose(a[rows], ref[key][rows], rtol=0, atol=atol, err_msg=f"{what}: {key}")
    return got


def rollout(backend, cfg_d, fast, E, steps, seed, mutate=None, actions=None, compare_wrecks=False, stats=None):
    """`steps` policy steps of `E` stream-identical spawns on an engine and on the oracle, free running, compared after every step.
    Linear traffic: the spawn's parameters go to both; direct control: the ids are DiscreteAction's, the stored controls start at
    zero on both and are compared with the state; Lidar: the observation is compared with the oracle's trace of the engine's own
    state (assert_lidar_of_own_state), the dynamics like everywhere else.  `stats` (dict): adds the live env-steps ("live"), those
    compared in full ("full") and those under the one exclusion (comparable) ("excluded").  `backend` None: the oracle alone -- nothing
    is compared, `stats` counts what a comparison of these draws WOULD cover (the exclusion is a condition on the oracle's own
    margin, so the coverage of a fuzz family is known before any kernel is involved)."""
    cfg = _abi.make_config(cfg_d, E, fast=fast)
    st = spawn.spawn_reference_stream(cfg, np.arange(E) + 100 * seed, cfg_d["ego_spacing"], cfg_d["vehicles_density"],
                                      cfg_d["initial_lane_id"])
    direct = cfg.ego_control == _abi.EGO_DIRECT
    if direct:
        oracle.zero_controls(cfg, st)
    if mutate:
        mutate(st)
    ref = _abi.copy_state(st)
    eng = make_engine(backend, cfg) if backend is not None else None
    if eng is not None:
        load_engine(eng, st)
    rng = np.random.default_rng(seed)
    live = np.ones(E, bool)
    for t in range(steps):
        acts = (rng.integers(0, _abi.num_actions(cfg), size=(E, cfg.num_agents)) if actions is None else np.full((E, cfg.num_agents), actions[t % len(actions)])).astype(np.int32)
        if eng is not None:
            obs, reward, term, trunc, info = eng.step(acts)
        with oracle.impact_margins(cfg) as m:
            o2, r2, te2, tr2, i2 = oracle.step(cfg, ref, acts)
        wreck, ok = comparable(ref, m.margin.min(1), live, compare_wrecks)
        if stats is not None:
            for key, n in (("live", live.sum()), ("full", ok.sum()), ("excluded", (live & ~ok).sum())):
                stats[key] = stats.get(key, 0) + int(n)
        if eng is None:
            live &= ~wreck
            continue
        got = compare_step(cfg, eng, (obs, reward, term, trunc), ref, (o2, r2, te2, tr2), wreck, ok, live, f"step {t}")
        live &= ~wreck
        if not live.all():  # keep dead envs in lock-step with the oracle so that live ones stay comparable
            for k in got:
                got[k][~live] = ref[k][~live]
            eng.set_state(got)
            if direct:
                a, s = (np.array(x, np.float64) for x in eng.get_controls())
                a[~live], s[~live] = ref["ctl_accel"][~live], ref["ctl_steer"][~live]
                eng.set_controls(a, s)
    if eng is not None:
        eng.close()
    return ref
