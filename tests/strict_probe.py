"""``python -m tests.strict_probe <backend> <out.npz> --row LABEL [--from FUSED.npz]``: one row of the fused-against-strict
comparison of tests/test_strict_arithmetic.py, run in a process of its own because the build a process runs is chosen when it
starts (tests/strict_util.py).

* without ``--from`` (the product's arithmetic): a device reset with fixed seeds, auto-reset on, then T policy steps with fixed
  random actions.  Before every step the state the engine steps from is recorded.
* with ``--from`` (the strict build): NO reset -- the spawn arithmetic contracts too, a strict reset would start from other last
  bits.  Before every step the engine is set to the state the fused run recorded there (and its extras: behaviour parameters, stored
  controls), so that each step of the two builds starts from IDENTICAL inputs; the re-spawn of an ended episode is taken from a
  launch of its own (run_strict).  The episode counters need no hand-over: both start
  at zero (a reset zeroes them, an engine is created with zeros) and advance where an episode ends, which the comparison holds
  equal; the auto-reset streams are a function of (base seed, environment, episode).

Both write, for every step: the state stepped from (``pre/``), the outputs (``out/``), get_state() after it (``post/``) and
variants_util.extras() before and after (``pre_x/``, ``post_x/``), each stacked over the steps; the strict run also which
environments the step re-spawned (``respawned``).

``--math``: instead of a row, the values of the probe ops of hwy_math.h on a fixed set of arguments (is tests/test_device_math.py's
subject the same bit for bit in two builds?) and of op 42, the arithmetic probe."""
from __future__ import annotations

import argparse

import numpy as np

from highwayenv_amd import _abi
from tests import variants_util as vu
from tests.families_util import load_engine

E, T = 32, 6
BASE_SEED = 77
OUT_KEYS = ("obs", "reward", "terminated", "truncated", "speed", "crashed")
ARITHMETIC_OP = 42  # hwy_device.h math_probe: x * x - 1.0 in one source expression


def merge_grid_row() -> dict:
    d = vu.merge_row()
    d["observation"] = {"type": "MultiAgentObservation", "observation_config": {"type": "OccupancyGrid"}}
    return d


SEED = 5


def rows() -> list:
    """(label, config dict, make_config keywords, seed): the smallest shapes that reach each kernel family -- eight rows of
    variants_util.rows(), and the three families in which the register-allocation knob selects nothing and which that table
    therefore leaves out: the wide kernel, OccupancyGrid on the road network, the intersection with more than 32 slots.  With the
    seed of the rows (device reset seeds 1000 * seed + e, auto-reset stream, actions) the ORACLE flags no env-step of any row as a
    push on the knife edge, on the emulator's and on the MI355X's record alike (tests/test_strict_arithmetic.py:
    test_fused_against_strict prints the count and holds it to 1 % of a row's env-steps)."""
    table = {r[0]: r for r in vu.rows()}
    picked = ["idm wave ego-only N=64", "idm wave full-scan N=64", "idm block NW=2 N=65", "linear wave full-scan N=64",
              "linear block NW=2 N=65", "direct wave full-scan N=64", "merge-generic Kinematics", "intersection N=30 helpers"]
    # (the table names the kernel a row's step() runs: highway-v0 on 4 lanes is the kernel compiled for it.  The row keeps its label
    # here: profiles/strict_arithmetic.md and the test ids carry it)
    in_table = {"idm wave full-scan N=64": "idm wave full-scan N=64 V0Shape4"}
    out = [(k, *table[in_table.get(k, k)][1:], SEED) for k in picked]
    out += [("idm wide N=101", vu.hwy(101), {}, SEED),
            ("merge-generic OccupancyGrid", merge_grid_row(), {"scenario": "merge-generic"}, SEED),
            ("intersection N=40", vu.ix(40), {"scenario": "intersection"}, SEED)]
    return out


def row(label: str):
    return next(r for r in rows() if r[0] == label)


def actions(cfg, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, _abi.num_actions(cfg), size=(T, cfg.num_envs, cfg.num_agents)).astype(np.int32)


def spawn_args(d: dict) -> dict:
    return {"ego_spacing": float(d.get("ego_spacing", 2.0)), "vehicles_density": float(d.get("vehicles_density", 1.0))}


def math_arguments() -> dict:
    """{probe op: arguments on the routine's domain} -- the scalar routines of hwy_math.h (ops 20 .. 33 evaluate them in pairs on
    arguments the probe itself computes with an a * x + b, which is the flag's business and not the routine's)."""
    rng = np.random.default_rng(7)
    n = 4096
    ang = rng.uniform(-np.pi, np.pi, n)
    return {0: np.exp(rng.uniform(-20, 20, n)), 1: rng.uniform(-700, 0, n), 2: ang, 3: ang, 4: rng.uniform(-1, 1, n),
            5: np.exp(rng.uniform(-10, 10, n)), 6: np.exp(rng.uniform(-10, 10, n)), 7: rng.uniform(-1e4, 1e4, n),
            8: rng.uniform(-50, 50, n), 9: rng.uniform(-50, 50, n), 10: rng.uniform(-50, 50, n), 11: rng.uniform(-50, 50, n),
            12: rng.uniform(-np.pi / 3, np.pi / 3, n)}


def arithmetic_arguments() -> np.ndarray:
    """x = 1 + 2^-k: x * x = 1 + 2^(1-k) + 2^(-2k) exactly, and the last term is below half an ulp of the product for k >= 27."""
    return 1.0 + 2.0 ** -np.arange(27, 40).astype(np.float64)


def run_math(backend: str, out: str) -> None:
    from tests.backends import make_engine
    eng = make_engine(backend, _abi.make_config(_abi.highway_fast_default_config(), 1, fast=True))
    data = {f"op{op}": eng.debug_math(op, x) for op, x in math_arguments().items()}
    data["arithmetic"] = eng.debug_math(ARITHMETIC_OP, arithmetic_arguments())
    eng.close()
    np.savez(out, **data)


def _record(rec: dict, prefix: str, arrays: dict) -> None:
    for k, v in arrays.items():
        rec.setdefault(f"{prefix}/{k}", []).append(np.array(v))


def _outputs(out) -> dict:
    obs, reward, term, trunc, info = out
    return dict(zip(OUT_KEYS, (obs, reward, term, trunc, info["speed"], info["crashed"])))


def run_fused(eng, d: dict, seed: int, acts) -> dict:
    rec = {}
    vu.reset_for_comparison(eng, d, 1000 * seed + np.arange(E), base_seed=BASE_SEED + seed)
    for t in range(T):
        _record(rec, "pre", eng.get_state())
        _record(rec, "pre_x", vu.extras(eng))
        _record(rec, "out", _outputs(eng.step(acts[t])))
        _record(rec, "post", eng.get_state())
        _record(rec, "post_x", vu.extras(eng))
    return rec


def run_strict(eng, d: dict, seed: int, acts, given: dict) -> dict:
    """Teacher-forced on the fused run's record `given`.  An environment whose episode ended in step t - 1 is RE-SPAWNED by step t
    instead of stepped, and what tells the kernel so -- the done flag the step kernel left -- is not part of a state: set_state
    clears it.  So step t is taken in two launches:

    1. where an episode ended in step t - 1: one step() WITHOUT a set_state.  The engine still holds the done flags its own step
       t - 1 left (taken from the fused run's state, so the same decision from the same inputs), re-spawns those environments from
       its own episode counters, and only THEIR rows of the outputs and of the state are kept ("respawned");
    2. set_state to the fused run's recorded state and step(): the rows of every other environment.  The rows of the re-spawned
       environments must leave no done flag behind in this launch (launch 1 of the next step would re-spawn an environment the
       fused run did not), so they are filled with an env-step of the fused run that is known not to end an episode: the state,
       the extras and the action of the first recorded env-step that neither re-spawned nor ended -- checked after the launch.

    This does not depend on what the seed makes the episodes do.  A re-spawn step itself never ends an episode (the kernel stores
    terminated = truncated = 0 for it).  An environment that ends its episode in the FIRST step after its re-spawn does so in
    launch 2 of that step, stepped from the recorded state like any other, leaves its done flag there and is re-spawned by launch 1
    of the step after (with the rows' seed: 24 episodes of an idm row end in a crash, several of them in their first step).  What
    the scheme needs is one env-step in the whole record that was stepped and did not end: asserted below."""
    rec = {}
    eng.set_autoreset(True, base_seed=BASE_SEED + seed, **spawn_args(d))
    ended = np.asarray(given["out/terminated"] | given["out/truncated"], bool)
    stepped = np.concatenate([np.ones((1, E), bool), ~ended[:-1]])
    assert (stepped & ~ended).any(), "the fused run holds no env-step that was stepped and did not end its episode: no filler"
    t0, e0 = np.argwhere(stepped & ~ended)[0]
    done = np.zeros(E, bool)
    for t in range(T):
        pre = {k.split("/", 1)[1]: v for k, v in given.items() if k.startswith(("pre/", "pre_x/"))}
        first = None
        if done.any():
            first = (_outputs(eng.step(acts[t])), eng.get_state(), vu.extras(eng))
        load_engine(eng, {k: np.ascontiguousarray(np.where(done.reshape(-1, *[1] * (v.ndim - 2)), v[t0][e0], v[t])) for k, v in pre.items()})
        acts_t = np.where(done[:, None], acts[t0][e0], acts[t]).astype(np.int32)
        st, ex = eng.get_state(), vu.extras(eng)
        out = _outputs(eng.step(acts_t))
        assert not (out["terminated"] | out["truncated"])[done].any(), \
            f"step {t}: a filler env-step ended its episode (environments {np.flatnonzero((out['terminated'] | out['truncated']) & done)})"
        post, post_x = eng.get_state(), vu.extras(eng)
        if first is not None:
            for mine, theirs in zip((out, post, post_x), first):
                for k in mine:
                    mine[k][done] = theirs[k][done]
        _record(rec, "pre", st)
        _record(rec, "pre_x", ex)
        _record(rec, "out", out)
        _record(rec, "post", post)
        _record(rec, "post_x", post_x)
        rec.setdefault("respawned", []).append(done.copy())
        done = np.asarray(out["terminated"] | out["truncated"], bool)
    return rec


def run_row(backend: str, out: str, label: str, fused: str | None) -> None:
    _, d, kw, seed = row(label)
    eng = vu.make_engine(backend, d, kw, E)
    acts = actions(eng.cfg, seed)
    if fused is None:
        rec = run_fused(eng, d, seed, acts)
    else:
        with np.load(fused) as z:
            rec = run_strict(eng, d, seed, acts, {k: z[k] for k in z.files})
    if hasattr(eng, "counters"):  # (the product; the emulation keeps no counters)
        assert eng.counters()["nonfinite_stores"] == 0
    eng.close()
    np.savez(out, actions=acts, **{k: np.stack(v) for k, v in rec.items()})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("backend", choices=["emu", "hip"])
    ap.add_argument("out")
    ap.add_argument("--row")
    ap.add_argument("--from", dest="fused")
    ap.add_argument("--math", action="store_true")
    a = ap.parse_args()
    if a.math:
        run_math(a.backend, a.out)
    else:
        run_row(a.backend, a.out, a.row, a.fused)
