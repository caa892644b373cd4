"""The yardstick of every device spawn of the straight road (hwy_reset and the re-spawn branch of the step and rollout kernels),
independent of the kernel source: Philox-4x32-10 restated in Python (pinned to the published known answers by
tests/test_spawn_paths.py), the draws of a vehicle laid out as the kernels consume them (counter = vehicle, episode, draw, 'HWY1';
key = the environment's seed), and the spawn RULE of the reference as array arithmetic -- ``spawn.spawn_from_draws`` /
``spawn.behavior_from_draws``, themselves pinned to the unmodified reference's own reset states (tests/test_spawn.py,
tests/test_traffic_host.py).  Nothing here is compiled from highwayenv_amd/csrc.

``assert_spawned`` is the one checker of a spawned environment: state planes, time, the first observation, what a re-spawn step
returns, the Linear family's parameters and a direct-control ego's stored action."""
from __future__ import annotations

import numpy as np

from highwayenv_amd import _abi, spawn
from oracle import oracle
from tests.lidar_util import cells_off

M32 = 0xFFFFFFFF
STREAM_TAG = 0x48575931  # 'HWY1': counter word 3 of every draw of the spawn
INT_PLANES = ("lane", "target_lane", "flags", "speed_index")
F64_PLANES = ("x", "y", "heading", "speed", "target_speed", "timer", "delta")


def philox4x32_10(counter, key):
    """Philox-4x32-10 (Salmon et al. 2011, "Parallel random numbers: as easy as 1, 2, 3"): four 32-bit counter words and two key
    words in, four 32-bit words out."""
    c = [int(w) & M32 for w in counter]
    k0, k1 = int(key[0]) & M32, int(key[1]) & M32
    for _ in range(10):
        p0 = 0xD2511F53 * c[0]
        p1 = 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c[3] ^ k1) & M32, p0 & M32]
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return c


def philox_uniform2(seed, vehicle, episode, draw):
    """Two uniforms in [0, 1) with 53 bits each: counter (vehicle, episode, draw, 'HWY1'), key = seed."""
    c = philox4x32_10((vehicle, episode, draw, STREAM_TAG), (seed & M32, (seed >> 32) & M32))
    a, b = (c[0] << 32) | c[1], (c[2] << 32) | c[3]
    return (a >> 11) / 9007199254740992.0, (b >> 11) / 9007199254740992.0


def _episodes(episode, E):
    return np.broadcast_to(np.asarray(episode, np.int64), (E,))


def expected_state(cfg, seeds, episode, ego_spacing, density, initial_lane_id):
    """The spawn rule on the Python Philox draws 0 (lane, speed) and 1 (position, delta) of every vehicle; `episode`: one number, or
    one per environment."""
    E, N, L = len(seeds), cfg.num_vehicles, cfg.lanes_count
    episode = _episodes(episode, E)
    lane = np.zeros((E, N), np.int64)
    us, up, ud = np.zeros((E, N)), np.zeros((E, N)), np.zeros((E, N))
    ctrl = spawn.controlled_mask(cfg)
    for e, sd in enumerate(seeds):
        for i in range(N):
            u_lane, u_speed = philox_uniform2(int(sd), i, int(episode[e]), 0)
            u_pos, u_delta = philox_uniform2(int(sd), i, int(episode[e]), 1)
            lane[e, i] = min(int(u_lane * L), L - 1)
            if ctrl[i] and initial_lane_id >= 0:
                lane[e, i] = initial_lane_id
            us[e, i], up[e, i], ud[e, i] = u_speed, u_pos, u_delta
    return spawn.spawn_from_draws(cfg, lane, us, up, ud, ego_spacing, density)


def expected_behavior(cfg, seeds, episode):
    """``spawn.behavior_from_draws`` on the Python Philox draws 2, 3 and 4 of every vehicle, in the order (a0, a1), (a2, s0), (s1, -):
    the Linear family's parameters [E, N, 5] after a spawn (controlled vehicles: zeros)."""
    E, N = len(seeds), cfg.num_vehicles
    episode = _episodes(episode, E)
    u = np.zeros((E, N, _abi.HWY_BEHAVIOR_PARAMS))
    for e, sd in enumerate(seeds):
        for i in range(N):
            a0, a1 = philox_uniform2(int(sd), i, int(episode[e]), 2)
            a2, s0 = philox_uniform2(int(sd), i, int(episode[e]), 3)
            s1, _ = philox_uniform2(int(sd), i, int(episode[e]), 4)
            u[e, i] = [a0, a1, a2, s0, s1]
    return spawn.behavior_from_draws(cfg, u)


def assert_spawn_equal(got, want, rows=slice(None)):
    for k in INT_PLANES:
        np.testing.assert_array_equal(got[k][rows], want[k][rows], err_msg=k)
    for k in F64_PLANES:
        np.testing.assert_allclose(got[k][rows], want[k][rows], rtol=0, atol=1e-9, err_msg=k)


def expected_spawn(cfg, seeds, episodes, spawn_kw) -> dict:
    """The whole expected spawn of every environment as the oracle takes it: the state planes at time 0, the Linear family's
    parameters (``behavior``), a direct-control ego's stored action (zeros, ``Vehicle.__init__``)."""
    lane_id = spawn_kw.get("initial_lane_id", -1)
    st = expected_state(cfg, seeds, episodes, spawn_kw["ego_spacing"], spawn_kw["vehicles_density"], -1 if lane_id is None else lane_id)
    if cfg.traffic_model == _abi.TRAFFIC_LINEAR:
        st["behavior"] = expected_behavior(cfg, seeds, episodes)
    if cfg.ego_control == _abi.EGO_DIRECT:
        oracle.zero_controls(cfg, st)
    return st


def assert_spawn_outputs(cfg, want, rows, outputs, what="spawn", eng=None) -> None:
    """What the call that spawned environments `rows` returned for them, against the expected spawn `want` (``expected_spawn``):
    `outputs` is the observation alone (``reset``) or the five outputs of a re-spawn step (of ``step``, or of one step of a
    ``rollout``).  `eng`: the engine, while it still holds that spawn (a Lidar observation is then also held to the oracle's
    trace of the engine's own state)."""
    from tests.families_util import assert_lidar_of_own_state
    from tests.golden_util import assert_obs_close
    obs = outputs if isinstance(outputs, np.ndarray) else outputs[0]
    want_obs = oracle.observe(cfg, want)
    if cfg.obs_type == _abi.OBS_LIDAR:
        if eng is not None:
            assert_lidar_of_own_state(cfg, eng, obs, what, rows=rows)
        off = cells_off(obs[rows], want_obs[rows])
        assert off == 0, f"{what}: {off} lidar cells beyond 1e-6 of the oracle's trace of the expected spawn"
    else:
        assert_obs_close(obs[rows], want_obs[rows], bool(cfg.flags & _abi.C_GRID_IMAGE), what, atol=1e-6)
    if not isinstance(outputs, np.ndarray):
        _, reward, term, trunc, info = outputs
        agents = list(cfg.agent_index[:cfg.num_agents])
        assert (reward[rows] == 0.0).all(), f"{what}: reward {reward[rows]}"
        assert not term[rows].any() and not trunc[rows].any(), f"{what}: a re-spawn step ended an episode"
        assert not info["crashed"][rows].any(), f"{what}: crashed"
        np.testing.assert_array_equal(info["speed"][rows], want["speed"][rows][:, agents], err_msg=f"{what}: info speed")


def assert_spawned(cfg_d, cfg, eng, rows, seeds, episodes, outputs, spawn_kw, what="spawn", stats=None) -> dict:
    """Environments `rows` of `eng` hold, right now, the spawn of (`seeds`[e], `episodes`[e]) under `spawn_kw` (ego_spacing,
    vehicles_density, initial_lane_id as the engine was given them; what is missing is the configuration dict `cfg_d`'s), and
    `outputs` is what the call that spawned them returned for them: the observation alone (``reset``), or the five outputs of a
    ``step`` that re-spawned them.

    * state: integer planes exact, f64 planes at 1e-9 (``assert_spawn_equal``), ``time == 0``;
    * observation: ``oracle.observe`` of the EXPECTED state at 1e-6 (Kinematics, OccupancyGrid); Lidar: no cell beyond 1e-6 of the
      oracle's trace of the expected state, nor of the engine's own state;
    * a re-spawn step: reward exactly 0, terminated / truncated / crashed False, ``info["speed"]`` the ego's spawned speed;
    * Linear traffic: ``get_behavior()`` bit-equal to ``expected_behavior`` (controlled rows zero);
    * direct control: ``get_controls()`` exactly zero.

    `seeds`, `episodes`: one per environment of the engine (only `rows` are read).  `stats` (dict): "dx" becomes the largest
    |x - expected x| seen.  Returns the expected spawn of all environments (``expected_spawn``; rows outside `rows` hold the spawn
    their seed and episode WOULD give)."""
    E = cfg.num_envs
    rows = np.flatnonzero(rows) if np.asarray(rows).dtype == bool else np.asarray(rows, np.intp)
    spawn_kw = {**{k: cfg_d[k] for k in ("ego_spacing", "vehicles_density", "initial_lane_id")}, **spawn_kw}
    want = expected_spawn(cfg, [int(s) for s in np.asarray(seeds).reshape(E)], _episodes(episodes, E), spawn_kw)
    if rows.size == 0:
        return want
    got = eng.get_state()
    if stats is not None:
        stats["dx"] = max(stats.get("dx", 0.0), float(np.abs(got["x"][rows] - want["x"][rows]).max()))
    try:
        assert_spawn_equal(got, want, rows)
    except AssertionError as ex:
        raise AssertionError(f"{what}: environments {rows.tolist()}\n{ex}") from ex
    assert (got["time"][rows] == 0).all(), f"{what}: time {got['time'][rows]}"
    assert_spawn_outputs(cfg, want, rows, outputs, what, eng)
    if cfg.traffic_model == _abi.TRAFFIC_LINEAR:
        b = eng.get_behavior()
        np.testing.assert_array_equal(b[rows], want["behavior"][rows], err_msg=f"{what}: behaviour parameters")
        assert not b[rows][:, spawn.controlled_mask(cfg)].any(), f"{what}: parameters of a controlled vehicle"
    if cfg.ego_control == _abi.EGO_DIRECT:
        accel, steer = eng.get_controls()
        assert not np.asarray(accel)[rows].any() and not np.asarray(steer)[rows].any(), f"{what}: stored controls"
    return want
