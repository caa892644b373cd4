"""The step kernels compiled for the registered configurations (csrc/hwy_wave.h: hwy_shape_wave_kernel<FixedShape<...>, WPE>) against
the ORACLE, free running, with auto-reset on -- the launches every other oracle comparison of the suite never takes (they run
without auto-reset, i.e. on the generic kernel: csrc/hwy_launch_family.h, step_shape_of).

``autoreset_rollout`` is ``families_util.rollout`` with the device's auto-reset: 8 stream-identical spawns, random actions, episodes
of 4 policy steps in twice the default density, the oracle compared after every step with ``families_util.compare_step`` at its
tolerances.  An environment that ended is re-spawned by the kernel on the next step; the oracle adopts the engine's state of those
rows after that step and they are compared again from there on, so the traffic the kernel spawned is held to the oracle too (the
spawn itself: tests/test_spawn_paths.py).  An environment that holds a wreck without having ended (a pile-up of traffic on
highway-v0) rests, like in ``rollout``, until its episode is over and the kernel re-spawns it.  After every step the library must
report the shape's kernel (hwy_last_step_shape).

What the inputs exercise is a condition on the ORACLE'S OWN run of the same draws (``backend=None``: ended environments take the
expected spawn of tests/spawn_util.py), asserted before any kernel is involved: the one exclusion of ``comparable`` removes no live
env-step; at N >= 12 the run holds an ego crash, a truncation followed by a re-spawn and FASTER on the top rung of the speed
ladder; for highway-v0 (the shape that keeps the full pairwise scan) a collision between two vehicles of the traffic.  N = 1 is the
ego alone (every other observation row zeroed), N = 3 fewer vehicles than observation rows, N = 64 a wavefront without an idle lane.
On the MI355X the N = 64 runs are repeated on the 1- and 4-wave register-allocation builds."""
import functools

import numpy as np
import pytest

from highwayenv_amd import _abi, spawn
from oracle import oracle
from tests import spawn_util
from tests import variants_util as vu
from tests.families_util import comparable, compare_step, make_engine

E, STEPS, DURATION, DENSITY = 8, 12, 4, 2.0
FASTER = 3
KINDS = {"fast-3": 1, "fast-4": 2, "v0-4": 3}  # hwy_last_step_shape of FastShape3, FastShape4, V0Shape4
SIZES = (1, 3, 12, 64)
# One seed per (shape, N) -- the spawn stream, the auto-reset stream and the actions derive from it -- for which the oracle's own run
# meets the conditions above: the smallest that does, found on the CPU (profiles/step_shape_coverage.md has the counts)
SEEDS = {
    ("fast-3", 1): 1, ("fast-3", 3): 1, ("fast-3", 12): 2, ("fast-3", 64): 11,
    ("fast-4", 1): 1, ("fast-4", 3): 1, ("fast-4", 12): 4, ("fast-4", 64): 4,
    ("v0-4", 1): 1, ("v0-4", 3): 1, ("v0-4", 12): 67, ("v0-4", 64): 2,
}


def config(kind: str, n: int, tuning=None):
    """(config dict, fast) of a registered configuration with n vehicles in all, short episodes and dense traffic."""
    fast = kind != "v0-4"
    d = _abi.highway_fast_default_config() if fast else _abi.highway_default_config()
    d.update({"vehicles_count": n - 1, "lanes_count": 3 if kind == "fast-3" else 4, "vehicles_density": DENSITY, "duration": DURATION})
    if tuning:
        d["tuning"] = dict(tuning)
    return d, fast


def autoreset_rollout(backend, cfg_d, fast, seed, shape, stats):
    """STEPS policy steps of E stream-identical spawns on an engine under auto-reset and on the oracle, compared after every step;
    `backend` None: the oracle alone.  `stats`: live / full / excluded env-steps as in families_util.rollout, the re-spawns, and
    the events of the oracle's run on live rows."""
    cfg = _abi.make_config(cfg_d, E, fast=fast)
    assert vu.step_shape(cfg_d, {"fast": fast}) == shape
    kw = {"ego_spacing": float(cfg_d["ego_spacing"]), "vehicles_density": float(cfg_d["vehicles_density"]), "initial_lane_id": -1}
    st = spawn.spawn_reference_stream(cfg, np.arange(E) + 100 * seed, cfg_d["ego_spacing"], cfg_d["vehicles_density"],
                                      cfg_d["initial_lane_id"])
    ref = _abi.copy_state(st)
    base = 7000 + seed
    seeds = [base + e for e in range(E)]
    eng = None
    if backend is not None:
        eng = make_engine(backend, cfg)
        eng.set_state(st)
        eng.set_autoreset(True, base_seed=base, **kw)
    rng = np.random.default_rng(seed)
    live, done_prev, episode = np.ones(E, bool), np.zeros(E, bool), np.zeros(E, np.int64)
    for key in ("live", "full", "excluded", "respawns", "ego crash", "truncation then re-spawn", "FASTER on the top rung",
                "traffic collision"):
        stats.setdefault(key, 0)
    try:
        for t in range(STEPS):
            what = f"step {t}"
            acts = rng.integers(0, _abi.num_actions(cfg), size=(E, cfg.num_agents)).astype(np.int32)
            respawned = done_prev
            now = live & ~respawned   # compared in this step
            top = ref["speed_index"][:, 0] == cfg.num_target_speeds - 1
            if eng is not None:
                out = eng.step(acts)
                assert vu.last_step_shape(eng) == shape, f"{what}: the launch ran shape {vu.last_step_shape(eng)}"
            with oracle.impact_margins(cfg) as m:
                o2, r2, te2, tr2, i2 = oracle.step(cfg, ref, acts)
            wreck, ok = comparable(ref, m.margin.min(1), now)
            crashed = (ref["flags"] & _abi.F_CRASHED) != 0
            stats["live"] += int(now.sum())
            stats["full"] += int(ok.sum())
            stats["excluded"] += int((now & ~ok).sum())
            stats["respawns"] += int(respawned.sum())
            stats["ego crash"] += int((ok & te2 & crashed[:, 0]).sum())
            stats["truncation then re-spawn"] += int((now & tr2).sum()) if t + 1 < STEPS else 0
            stats["FASTER on the top rung"] += int((now & top & (acts[:, 0] == FASTER)).sum())
            stats["traffic collision"] += int((ok & ~crashed[:, 0] & (crashed[:, 1:].sum(1) >= 2)).sum())
            if eng is not None:
                got = compare_step(cfg, eng, out[:4], ref, (o2, r2, te2, tr2), wreck, ok, now, what, trunc_rows=now)
                ended = np.asarray(out[2] | out[3], bool)
                assert not ended[respawned].any(), f"{what}: a re-spawn step ended an episode"
            else:
                ended = te2 | tr2
                ended[respawned] = False
            # the rows this step re-spawned: the oracle goes on from the engine's spawn (the oracle alone: from the expected one)
            episode += respawned
            if respawned.any():
                fresh = got if eng is not None else spawn_util.expected_spawn(cfg, seeds, episode, kw)
                if eng is not None:
                    assert (got["time"][respawned] == 0).all(), f"{what}: time of a re-spawned environment"
                for k in ref:
                    ref[k][respawned] = fresh[k][respawned]
                ref["time"][respawned] = 0
            live = (now & ~wreck & ~ended) | respawned
            done_prev = ended
    finally:
        if eng is not None:
            eng.close()
    return stats


@functools.lru_cache(maxsize=None)
def oracle_alone(kind: str, n: int) -> dict:
    """The oracle's own run of a case, once per session: the conditions on the inputs, and the counts an engine's run must repeat."""
    d, fast = config(kind, n)
    stats = autoreset_rollout(None, d, fast, SEEDS[kind, n], KINDS[kind], {})
    assert stats["excluded"] == 0 and stats["full"] == stats["live"] > 0, stats
    assert stats["respawns"] >= E, stats   # (episodes last 4 steps: every environment is re-spawned twice in 12)
    if n >= 12:
        for event in ("ego crash", "truncation then re-spawn", "FASTER on the top rung"):
            assert stats[event] > 0, f"{kind} N={n}: the oracle's run shows no {event}: {stats}"
        if kind == "v0-4":
            assert stats["traffic collision"] > 0, f"{kind} N={n}: no collision between two vehicles of the traffic: {stats}"
    return stats


def _cases():
    out = []
    for kind in KINDS:
        for n in SIZES:
            out.append(pytest.param("emu", kind, n, None, id=f"emu-{kind}-N{n}"))
            out.append(pytest.param("hip", kind, n, None, id=f"hip-{kind}-N{n}", marks=pytest.mark.gpu))
        for w in (1, 4):   # the extreme register-allocation builds, held to the oracle directly
            out.append(pytest.param("hip", kind, 64, w, id=f"hip-{kind}-N64-wpe{w}", marks=pytest.mark.gpu))
    return out


@pytest.mark.parametrize("backend,kind,n,wpe", _cases())
def test_shape_kernel_vs_oracle_under_autoreset(backend, kind, n, wpe):
    want = oracle_alone(kind, n)
    d, fast = config(kind, n, {"waves_per_eu": wpe} if wpe else None)
    got = autoreset_rollout(backend, d, fast, SEEDS[kind, n], KINDS[kind], {})
    # the engine's run compared what the oracle's own run promised: no environment went missing on the way
    assert got == want, (got, want)
