"""Every kernel path that spawns a straight road, held to the reference's spawn rule on Philox uniforms computed in Python
(tests/spawn_util.py -- nothing of the yardstick is compiled from the kernel source): the three reset kernels, and the re-spawn
branch of the one-wavefront kernel (N <= 64), of the wide kernel (IDM traffic, K = 2 vehicles per thread for 64 < N <= 128 as the
engine chooses it, K = 3 and 4 for 128 < N <= 256 under ``tuning={"block_kernel": 2}``) and of the workgroup kernel
(``block_kernel`` 1, and the engine's choice for IDM beyond 128 vehicles; the Linear family and direct control beyond 64 vehicles),
in their step and rollout builds.  Backends: ``emu`` = the CPU emulation of the kernel source, ``hip`` = the MI355X.

One parametrised test over ROWS; each row is the smallest shape that selects a path or an edge, and is driven through three entry
points:

(a) ``reset(seeds=...)`` on every environment, ``reset(mask=..., seeds=...)`` on a strict subset with new seeds (the other rows stay
    bit-identical) and ``reset(base_seed=...)``;
(b) auto-reset with ``duration`` 2 at policy frequency 1 and 8 calls of ``step()`` with random actions: after every step the rows
    that were done before it are held to the spawn of their next episode (``spawn_util.assert_spawned``), and the rows spawned by
    the call before are compared with ``oracle.step`` from the EXPECTED spawn (``families_util.compare_step``, its tolerances and
    its one exclusion) -- that step reads the rank hint ``spawn_fill`` wrote.  Then a masked ``reset`` in the middle of the run
    restarts the episode count of its rows only: three steps later they are on episode 1 again, the others on 3 or 4;
(c) the first 6 steps of (b) as ONE ``rollout()`` on a second engine: the outputs of every re-spawn row of every step, and the
    final state of the environments whose last step was a re-spawn.

Coverage is a condition, not a hope: an episode lasts at most two steps, so every environment is re-spawned at least twice
(episodes 1 and 2) within the first 7 steps of (b) and within the 6 of (c); the test asserts both.  Run with ``-s`` for each row's
re-spawn counts and largest |x - expected x|."""
import numpy as np
import pytest

from highwayenv_amd import _abi
from oracle import oracle
from tests import spawn_util
from tests.backends import BACKENDS
from tests.families_util import comparable, compare_step, engine_state, make_engine

BEHAVIOR = "highway_env.vehicle.behavior."
LIDAR = {"type": "LidarObservation", "cells": 16, "maximum_range": 60}
GRID = {"type": "OccupancyGrid", "features": ["presence", "vx", "vy", "cos_h", "on_road"], "grid_size": [[-40, 40], [-12, 12]],
        "grid_step": [8, 4]}


def _row(family, total, lanes, agents, lane, fast, ego_spacing, density, bk=None, **extra):
    """family: idm | Aggressive | Defensive (Linear traffic of that class) | direct, with an optional -lidar / -grid observation;
    total: N, agents included; lane: initial_lane_id -- None, 0 or "last" (L - 1); bk: tuning block_kernel (None = not set)."""
    name = f"{family}-n{total}-l{lanes}-a{agents}" + ("" if bk is None else f"-bk{bk}") + ("-fast" if fast else "")
    return pytest.param(dict(family=family, total=total, lanes=lanes, agents=agents, lane=lane, fast=fast, ego_spacing=ego_spacing,
                             density=density, bk=bk, **extra), id=name)


# IDM with meta-actions: every boundary of waves_for (K = 1 | 2 | 3 | 4 at 64 | 128 | 192), N = 1 (vehicles_count 0) and the maximum;
# each size on the engine's own choice of kernel (block_kernel 0: one wavefront for N <= 64, the wide kernel with K = 2 for
# 64 < N <= 128, the workgroup kernel beyond) and on the workgroup kernel (block_kernel 1)
#           N  lanes agents lane  fast  ego_spacing density
IDM = [(1, 1, 1, None, True, 1.7, 1.3), (2, 6, 2, 0, False, 2.5, 0.8), (63, 3, 3, "last", True, 1.0, 2.0),
       (64, 1, 1, 0, False, 1.7, 1.3), (65, 6, 2, "last", True, 2.5, 0.8), (127, 2, 3, None, False, 1.0, 2.0),
       (128, 4, 1, 0, True, 1.7, 1.3), (129, 5, 2, "last", False, 2.5, 0.8), (191, 3, 3, None, True, 1.0, 2.0),
       (192, 6, 1, 0, False, 1.7, 1.3), (193, 4, 2, "last", True, 2.5, 1.2), (255, 5, 3, None, False, 1.0, 2.0),
       (256, 6, 1, "last", True, 1.7, 1.3)]
# (block_kernel 0 beyond 128 vehicles is the workgroup kernel too -- the engine's choice there, hwy_params.h -- so the wide kernel
# with K = 3 and 4 vehicles per thread, its step and rollout builds, runs in the block_kernel 2 rows)
ROWS = [_row("idm", *r, bk=bk) for r in IDM for bk in ((0, 1) if r[0] <= 128 else (0, 1, 2))]
# a ladder of two target speeds, neither of them the ego's 25 m/s: the snap to the nearest entry clips (wide kernel, K = 2)
ROWS += [_row("idm", 70, 3, 2, None, True, 1.5, 1.0, target_speeds=[10, 20])]
# Linear traffic (the parameter ranges are the family's, not the class's) and DiscreteAction: one wavefront | the workgroup kernel
for fam_a, fam_b in (("Aggressive", "Defensive"), ("direct", "direct")):
    ROWS += [_row(fam_a, 2, 1, 1, None, True, 1.7, 1.3, bk=bk) for bk in (0, 1)]
    ROWS += [_row(fam_b, 64, 4, 2, 0, False, 2.5, 0.8, bk=bk) for bk in (0, 1)]
    ROWS += [_row(fam_a, 65, 6, 1, "last", True, 1.0, 2.0), _row(fam_b, 129, 3, 3, None, False, 1.7, 1.3),
             _row(fam_a, 256, 5, 1, 0, True, 2.5, 1.2)]
# the first observation of a spawn through the Lidar kernel (beside IDM and Linear traffic) and as an OccupancyGrid, beyond 64
ROWS += [_row("idm-lidar", 130, 4, 1, None, True, 1.5, 1.5), _row("Defensive-lidar", 70, 3, 2, 0, True, 1.5, 1.5),
         _row("idm-grid", 100, 4, 1, "last", True, 1.5, 1.5, bk=1)]

SEED_HIGH = (1 << 40) + (1 << 33)   # (seeds with bits above 2^32: both key words of the Philox are in play)


def row_config(row):
    """(cfg_d, fast, E, spawn_kw) of a row."""
    fast = row["fast"]
    d = _abi.highway_fast_default_config() if fast else _abi.highway_default_config()
    family, _, obs = row["family"].partition("-")
    A, L = row["agents"], row["lanes"]
    d.update({"vehicles_count": row["total"] - A, "lanes_count": L, "controlled_vehicles": A, "duration": 2, "policy_frequency": 1,
              "ego_spacing": row["ego_spacing"], "vehicles_density": row["density"],
              "initial_lane_id": {None: None, 0: 0, "last": L - 1}[row["lane"]]})
    if row["bk"] is not None:
        d["tuning"] = {"block_kernel": row["bk"]}
    act = {"type": "DiscreteMetaAction"}
    if "target_speeds" in row:
        act["target_speeds"] = row["target_speeds"]
    if family == "direct":
        act = {"type": "DiscreteAction", "steering_range": [-0.1, 0.1]}
    elif family != "idm":
        d["other_vehicles_type"] = BEHAVIOR + family + "Vehicle"
    observation = {"lidar": LIDAR, "grid": GRID, "": d["observation"]}[obs]
    if A > 1:
        act = {"type": "MultiAgentAction", "action_config": act}
        observation = {"type": "MultiAgentObservation", "observation_config": observation}
    d["action"], d["observation"] = act, observation
    E = 7 if row["total"] <= 128 else 3   # odd: a kernel that packs several environments per workgroup gets a partial last block
    kw = dict(ego_spacing=d["ego_spacing"], vehicles_density=d["vehicles_density"],
              initial_lane_id=-1 if d["initial_lane_id"] is None else d["initial_lane_id"])
    return d, fast, E, kw


def _assert_rows_untouched(before, after, rows, what):
    for k in before:
        np.testing.assert_array_equal(after[k][rows], before[k][rows], err_msg=f"{what}: {k} of an environment outside the mask")


class Run:
    """Entry point (b): an engine under auto-reset, stepped with random actions, with the bookkeeping of what each environment
    must hold: its episode, whether it was done before this step, and -- for the rows the previous call spawned -- the expected
    spawn the oracle steps from."""

    def __init__(self, cfg_d, cfg, eng, kw, base, ref, stats):
        self.cfg_d, self.cfg, self.eng, self.kw, self.stats = cfg_d, cfg, eng, kw, stats
        E = cfg.num_envs
        self.seeds = np.uint64(base) + np.arange(E, dtype=np.uint64)
        self.ref = ref                       # expected pre-step state of the rows in `fresh` (other rows: not compared)
        self.fresh = np.ones(E, bool)        # spawned by the previous call
        self.done_prev = np.zeros(E, bool)
        self.episode = np.zeros(E, np.int64)
        self.respawns = np.zeros(E, np.int64)
        self.stepped_on = np.zeros(E, np.int64)   # per environment: steps from an expected spawn compared with the oracle in full
        self.actions = []

    def step(self, acts, what):
        cfg, eng, ref = self.cfg, self.eng, self.ref
        self.actions.append(acts)
        out = eng.step(acts)
        # one step further: the rows spawned by the previous call, against the oracle from the expected spawn
        with oracle.impact_margins(cfg) as m:
            ref_out = oracle.step(cfg, ref, acts)
        wreck, ok = comparable(ref, m.margin.min(1), self.fresh)
        compare_step(cfg, eng, out[:4], ref, ref_out[:4], wreck, ok, self.fresh, f"{what}, the step after a spawn", trunc_rows=self.fresh)
        self.stepped_on += ok
        # the rows this step re-spawned
        rows = self.done_prev
        self.episode += rows
        self.respawns += rows
        want = spawn_util.assert_spawned(self.cfg_d, cfg, eng, rows, self.seeds, self.episode, out, self.kw, what, self.stats)
        for k in ref:
            ref[k][rows] = want[k][rows]
        self.fresh = rows.copy()
        self.done_prev = np.asarray(out[2] | out[3], bool)
        return out


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("row", ROWS)
def test_every_spawn_path_follows_the_reference_rule(backend, row):
    cfg_d, fast, E, kw = row_config(row)
    cfg = _abi.make_config(cfg_d, E, fast=fast)
    direct = cfg.ego_control == _abi.EGO_DIRECT
    everyone = np.ones(E, bool)
    stats = {}
    rng = np.random.default_rng(row["total"] * 7 + row["lanes"])
    eng = make_engine(backend, cfg)

    # ---- (a) reset: all environments, a strict subset, base_seed ---------------------------------------------------------------
    seeds0 = np.uint64(SEED_HIGH) + np.arange(E, dtype=np.uint64) * np.uint64(7919) + np.uint64(3)
    if direct:
        eng.set_controls(np.full((E, cfg.num_agents), 3.0), np.full((E, cfg.num_agents), 0.25))
    obs = eng.reset(seeds=seeds0, **kw)
    spawn_util.assert_spawned(cfg_d, cfg, eng, everyone, seeds0, 0, obs, kw, "reset(seeds)", stats)
    if direct:
        eng.set_controls(np.full((E, cfg.num_agents), -2.0), np.full((E, cfg.num_agents), 0.125))
    before = engine_state(eng)
    mask = np.zeros(E, bool)
    mask[1::2] = True
    seeds1 = seeds0 + np.uint64(1 << 34)
    obs = eng.reset(seeds=seeds1, mask=mask.astype(np.uint8), **kw)
    _assert_rows_untouched(before, engine_state(eng), ~mask, "reset(mask)")
    spawn_util.assert_spawned(cfg_d, cfg, eng, mask, seeds1, 0, obs, kw, "reset(mask, seeds)", stats)
    base0 = SEED_HIGH + 4242
    obs = eng.reset(base_seed=base0, **kw)
    ref = spawn_util.assert_spawned(cfg_d, cfg, eng, everyone, base0 + np.arange(E), 0, obs, kw, "reset(base_seed)", stats)

    # ---- (b) auto-reset, step by step ------------------------------------------------------------------------------------------
    base = SEED_HIGH + 99991
    eng.set_autoreset(True, base_seed=base, **kw)
    run = Run(cfg_d, cfg, eng, kw, base, ref, stats)
    n_act = _abi.num_actions(cfg)
    for t in range(7):
        run.step(rng.integers(0, n_act, size=(E, cfg.num_agents)).astype(np.int32), f"step {t}")
    respawns_b = run.respawns.copy()
    assert (respawns_b >= 2).all(), f"(b): re-spawns per environment {respawns_b}"
    run.step(rng.integers(0, n_act, size=(E, cfg.num_agents)).astype(np.int32), "step 7")  # (one step further for the rows step 6 spawned)
    # a masked reset in the middle of the run: the episode count of ITS rows restarts (the re-spawn seeds stay the auto-reset's)
    before = engine_state(eng)
    obs = eng.reset(seeds=seeds1, mask=mask.astype(np.uint8), **kw)
    _assert_rows_untouched(before, engine_state(eng), ~mask, "reset(mask) under auto-reset")
    want = spawn_util.assert_spawned(cfg_d, cfg, eng, mask, seeds1, 0, obs, kw, "reset(mask) under auto-reset", stats)
    for k in run.ref:
        run.ref[k][mask] = want[k][mask]
    run.fresh, run.episode[mask], run.done_prev[mask] = run.fresh | mask, 0, False
    for t in range(8, 11):
        run.step(rng.integers(0, n_act, size=(E, cfg.num_agents)).astype(np.int32), f"step {t} (after a masked reset)")
    assert (run.episode[mask] == 1).all() and (run.episode[~mask] >= 3).all(), run.episode
    # (the one exclusion of compare_step is a push direction on the knife edge, decided by the oracle alone: it must not have emptied
    # the comparison of "one step further" for any environment)
    assert (run.stepped_on >= 1).all(), f"(b): steps from an expected spawn compared with the oracle in full, per environment {run.stepped_on}"
    eng.close()

    # ---- (c) the first 6 steps as one rollout on a second engine ---------------------------------------------------------------
    K = 6
    eng = make_engine(backend, cfg)
    eng.reset(base_seed=base0, **kw)
    eng.set_autoreset(True, base_seed=base, **kw)
    outs = eng.rollout(np.stack(run.actions[:K]))
    episode, respawns_c = np.zeros(E, np.int64), np.zeros(E, np.int64)
    done_prev = np.zeros(E, bool)
    seeds = np.uint64(base) + np.arange(E, dtype=np.uint64)
    for k in range(K):
        episode += done_prev
        respawns_c += done_prev
        out_k = tuple(o[k] for o in outs[:4]) + ({key: v[k] for key, v in outs[4].items()},)
        if k == K - 1:   # the state the launch left: the spawn of the environments whose last step was a re-spawn
            spawn_util.assert_spawned(cfg_d, cfg, eng, done_prev, seeds, episode, out_k, kw, f"rollout step {k}", stats)
        elif done_prev.any():
            want = spawn_util.expected_spawn(cfg, [int(s) for s in seeds], episode, kw)
            spawn_util.assert_spawn_outputs(cfg, want, np.flatnonzero(done_prev), out_k, f"rollout step {k}")
        done_prev = np.asarray(out_k[2] | out_k[3], bool)
    eng.close()
    assert (respawns_c >= 2).all(), f"(c): re-spawns per environment {respawns_c}"
    print(f"\nspawn paths [{backend}] {row['family']} N={cfg.num_vehicles} E={E} block_kernel={row['bk']}: re-spawns per environment (b) {respawns_b.min()}..{respawns_b.max()} "
          f"(c) {respawns_c.min()}..{respawns_c.max()}, {run.stepped_on.sum()} env-steps from an expected spawn == oracle "
          f"({run.stepped_on.min()}..{run.stepped_on.max()} per environment), "
          f"largest |dx| {stats['dx']:.2e}")


# ---- the yardstick's own generator ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("counter,key,output", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_python_philox_known_answers(counter, key, output):
    """The published known answers of Philox-4x32-10 (Random123's kat_vectors: zeros, all ones, the digits of pi)."""
    assert tuple(spawn_util.philox4x32_10(counter, key)) == output


def test_python_philox_uniforms_are_the_counter_layout_of_the_spawn():
    """philox_uniform2 = the generator on counter (vehicle, episode, draw, 'HWY1') and key (seed low, seed high), its four words
    taken in pairs as two 53-bit uniforms."""
    seed, vehicle, episode, draw = (0x299f31d0 << 32) | 0xa4093822, 0x243f6a88, 0x85a308d3, 0x13198a2e
    w = spawn_util.philox4x32_10((vehicle, episode, draw, spawn_util.STREAM_TAG), (0xa4093822, 0x299f31d0))
    u0, u1 = spawn_util.philox_uniform2(seed, vehicle, episode, draw)
    assert u0 == (((w[0] << 32) | w[1]) >> 11) * 2.0 ** -53 and u1 == (((w[2] << 32) | w[3]) >> 11) * 2.0 ** -53
    assert 0.0 <= u0 < 1.0 and 0.0 <= u1 < 1.0 and u0 != u1
