"""A second arithmetic for the parity contract: the kernels built WITHOUT contraction (-ffp-contract=off), held to the reference
next to the product, and the product held to that build decision by decision.

The product contracts every a*b+c of one source expression into a fused multiply-add (highwayenv_amd/build.py: FP_CONTRACT); the
reference's numpy scalars and the C oracle round the product and the sum separately.  DESIGN.md section 4 therefore rests every
exact comparison on the decisions being well conditioned, and holds the lateral offset of slow intersection cars at 1e-6 where
the unfused build of rounds 1-3 held 1e-8.  With one arithmetic in the suite a knife-edge carve-out that fires, or a slow-car
difference of 3e-8, cannot be told from an algorithmic difference that stays under a loosened bound.  Here:

1. an arithmetic probe (hwy_debug_math op 42: ``x * x - 1.0``) proves which build a library is: the product returns the fused
   value, the strict library (highwayenv_amd/build.py: build_engine_strict; the emulator under HWY_EMU_FLAGS) the double-rounded
   one -- a strict library that silently kept the product's flag would make everything below pass for nothing;
2. the strict library holds exactly the product's kernels, behind the same ABI;
3. the suite's comparisons with the reference's fixtures and with the oracle PASS on the strict build at the suite's tolerances,
   the intersection ones with the slow-car bound back at 1e-8 (HWY_STRICT_TOL=1, tests/golden_util.py) -- and that bound FAILS on
   the product's arithmetic, so it is able to fail at all;
4. fused against strict, teacher-forced (tests/strict_probe.py): from identical states one policy step of the two builds makes
   the SAME discrete decisions on every kernel family, floats within the suite's one-step tolerances;
5. one chunk of every fuzz family passes on the strict build under the existing ceilings; the tolerated-and-counted figures are
   printed, for the two-column ledger of profiles/strict_arithmetic.md.

Every run on the strict build is a child process (tests/strict_util.py); ``emu`` legs need no GPU, ``hip`` legs are marked gpu."""
import os
import re

import numpy as np
import pytest

from highwayenv_amd import _abi, build
from tests import strict_probe, strict_util
from tests.golden_util import KNIFE

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]


def _legs(cases, ident=lambda c: c[0]):
    """(backend, *case) for both backends, the hip ones marked gpu."""
    return ([pytest.param("emu", *c, id=f"emu-{ident(c)}") for c in cases]
            + [pytest.param("hip", *c, id=f"hip-{ident(c)}", marks=pytest.mark.gpu) for c in cases])


@pytest.fixture(scope="module")
def strict_lib():
    """libhwy_engine_strict.so: rebuilt only if it is missing or stale."""
    if build.is_stale():
        build.build_engine()
    return build.build_engine_strict()


def _load(path) -> dict:
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def _probe(backend, out, *args, strict, timeout):
    res = strict_util.run_child(backend, ["-m", "tests.strict_probe", backend, str(out), *args],
                                strict_util.child_env(backend, strict), timeout)
    assert res.returncode == 0, f"tests.strict_probe {backend} {args} (return code {res.returncode}):\n{res.stdout[-3000:]}\n{res.stderr[-3000:]}"
    return _load(out)


# --------------------------------------------------------------------------- 1. which arithmetic a library has

@pytest.mark.parametrize("backend", BACKENDS)
def test_the_product_fuses_and_the_strict_build_does_not(backend, tmp_path, request):
    """x = 1 + 2^-k, k = 27 .. 39: x * x - 1 is 2^(1-k) + 2^(-2k) in one rounding (both terms fit one double) and 2^(1-k) when the
    product is rounded first (2^(-2k) is below half an ulp of 1 + 2^(1-k)).  Printed, not asserted: on how many of 4096 arguments
    each scalar routine of hwy_math.h returns other bits in the two builds.  The routines fuse explicitly (fma()) where it matters
    to their error bound, but exp_bounded and the atan family also hold a few plain a*b+c that the flag decides -- both builds are
    held to the same ulp bounds by tests/test_device_math.py (the device_math selection below), which is the requirement."""
    if backend == "hip":
        request.getfixturevalue("strict_lib")
    fused = _probe(backend, tmp_path / "fused.npz", "--math", strict=False, timeout=300)
    strict = _probe(backend, tmp_path / "strict.npz", "--math", strict=True, timeout=300)
    k = np.arange(27, 40).astype(np.float64)
    np.testing.assert_array_equal(strict_probe.arithmetic_arguments(), 1.0 + 2.0 ** -k)
    np.testing.assert_array_equal(fused["arithmetic"], 2.0 ** (1 - k) + 2.0 ** (-2 * k), err_msg="the product does not contract x * x - 1.0")
    np.testing.assert_array_equal(strict["arithmetic"], 2.0 ** (1 - k), err_msg="the strict build contracts x * x - 1.0")
    differ = {op: int((fused[op].view(np.uint64) != strict[op].view(np.uint64)).sum()) for op in sorted(fused) if op != "arithmetic"}
    print(f"\nstrict arithmetic [{backend}]: probe op 42 fused on the product, double-rounded on the strict build; hwy_math.h routines "
          f"with values that differ between the builds: { {op: n for op, n in differ.items() if n} or 'none' } of {len(differ)} ops x 4096")
    assert len(differ) == 13


# --------------------------------------------------------------------------- 2. the same kernels behind the same ABI

def test_the_strict_library_holds_the_products_kernels(strict_lib):
    pytest.importorskip("msgpack")  # (the metadata note is msgpack: tests/test_kernel_variants.py)
    product, strict = build.kernel_resources(), build.kernel_resources(strict_lib)
    assert len(product) > 100 and set(strict) == set(product), sorted(set(strict) ^ set(product))


def test_the_strict_library_has_the_products_abi(strict_lib):
    """hwy_abi_version and hwy_config_size of the two libraries -- one library per process: each is asked in a child of its own."""
    code = "from highwayenv_amd import _lib; l = _lib.load(); print('abi', l.hwy_abi_version(), l.hwy_config_size())"
    seen = []
    for lib in (None, strict_lib):
        env = strict_util.child_env("emu", strict=False, extra={"HWY_ENGINE_LIB": lib} if lib else None)
        res = strict_util.run_child("emu", ["-c", code], env, timeout=120)
        assert res.returncode == 0, res.stderr[-2000:]
        seen.append(re.search(r"abi (\d+) (\d+)", res.stdout).groups())
    assert seen[0] == seen[1] == (str(_abi.HWY_ABI_VERSION), str(__import__("ctypes").sizeof(_abi.HwyConfig))), seen
    assert os.path.getsize(strict_lib) > 0 and strict_lib != build.LIB_PATH


# --------------------------------------------------------------------------- 3. the reference's fixtures on the strict build

# (id, pytest selection, HWY_STRICT_TOL, time limit of the child on emu / on hip in seconds): the tests that compare with fixtures
# recorded from the unmodified reference, or with the oracle from a given state.  The limits are some five times what the
# selections take (emu: the build of the strict emulator libraries included).
SELECTIONS = [
    ("engine_parity", ["tests/test_engine_parity.py", "-k", "teacher_forced_frames_vs_reference or free_running_episodes_vs_reference"], False, 1500, 300),
    ("collision_steps", ["tests/test_collision_steps.py"], False, 1500, 300),
    ("net_parity", ["tests/test_net_parity.py"], False, 1500, 300),
    ("ix_parity", ["tests/test_ix_parity.py"], True, 1500, 300),
    ("oracle_golden_intersection", ["tests/test_oracle_golden_intersection.py"], True, 1500, 300),
    ("traffic_parity", ["tests/test_traffic_parity.py"], False, 1500, 400),
    ("control_parity", ["tests/test_control_parity.py"], False, 1500, 400),
    ("lidar_parity", ["tests/test_lidar_parity.py"], False, 1500, 300),
    ("ttc_parity", ["tests/test_ttc_parity.py"], False, 1500, 400),
    ("occupancy_grid", ["tests/test_occupancy_grid.py"], False, 1500, 300),
    ("device_math", ["tests/test_device_math.py"], False, 900, 300),
]
# (the oracle against the fixtures involves no engine: one leg, with the knob)
_SELECTION_CASES = [c for c in _legs(SELECTIONS) if c.id != "hip-oracle_golden_intersection"]


@pytest.mark.parametrize("backend,name,selection,tol,limit_emu,limit_hip", _SELECTION_CASES)
def test_reference_fixtures_on_the_strict_build(backend, name, selection, tol, limit_emu, limit_hip, request):
    if backend == "hip":
        request.getfixturevalue("strict_lib")
    res = strict_util.run_selection(backend, selection, strict=True, tol=tol, timeout=limit_emu if backend == "emu" else limit_hip)
    n = strict_util.assert_all_passed(res, f"{name} on the strict {backend} build" + (" at HWY_STRICT_TOL=1" if tol else ""))
    print(f"\nstrict arithmetic [{backend}]: {name}: {n} passed" + (" with the slow-car bound at 1e-8" if tol else ""))


def test_the_tightened_bound_fails_on_the_fused_emulator():
    """The control of the knob: on the PRODUCT's arithmetic a yielding car of intersection_multi_agent3 ends a policy step 2.8e-8
    from the reference's trace (4.8e-8 on the GPU: tests/test_ix_parity.py), beyond the 1e-8 the knob sets -- the same selection
    passes on the strict emulator (the ix_parity leg above)."""
    selection = ["tests/test_ix_parity.py", "-k", "test_policy_steps_vs_reference and intersection_multi_agent3"]
    res = strict_util.run_selection("emu", selection, strict=False, tol=True, timeout=900)
    assert res.returncode == 1 and "AssertionError" in res.stdout and "below 2.0 m/s" in res.stdout, \
        f"the fused emulator was expected to miss 1e-8 (return code {res.returncode}):\n{res.stdout[-3000:]}"
    res = strict_util.run_selection("emu", selection, strict=False, tol=False, timeout=900)
    strict_util.assert_all_passed(res, "the same selection with the knob unset")


# --------------------------------------------------------------------------- 4. fused against strict, decision by decision

WRECK = _abi.F_CRASHED | _abi.F_HAS_IMPACT
STATE_ATOL, WRECK_ATOL, REWARD_ATOL, OBS_ATOL = 1e-7, 1e-6, 1e-9, 1e-6   # (tests/families_util.py: compare_step; one policy step)
MAX_EXCLUDED = 0.01


def _at(rec: dict, prefix: str, t: int) -> dict:
    return {k.split("/", 1)[1]: np.array(v[t]) for k, v in rec.items() if k.startswith(prefix + "/")}   # (copies: the oracle steps in place)


def oracle_knife_edges(d: dict, kw: dict, fused: dict):
    """(knife [T, E], hit [T, E]) from the ORACLE, stepped from the state the fused run recorded before each step:

    * knife: env-steps with a collision whose push direction hinges on |d.normal| < KNIFE (utils.py:232-236) -- the suite's rule
      for one policy step from identical state (tests/test_net_parity.py: _rollout_vs_oracle with drift 0, tests/test_ix_parity.py,
      tests/test_fuzz_configs.py).  These env-steps are EXCLUDED and counted against the cap; nothing else is.  In particular the
      road-network families' rule for wrecks that rest exactly touching (flag_margin < KNIFE) is NOT applied: the two builds are
      held to the same crash bits and the same pending impact on those slots too;
    * hit: env-steps in which the oracle saw a collision at all -- the collision steps, whose vehicles are held to 1e-6.

    An environment that the step re-spawns is not stepped: nothing of it is flagged."""
    from oracle import oracle, oracle_ix
    from tests.golden_util import ix_oracle_config, ix_oracle_state
    acts = fused["actions"]
    T, E = acts.shape[:2]
    ix = kw.get("scenario") == "intersection"
    if ix:
        dh = dict(d, host_traffic=True)
        cfg = _abi.make_config(dh, E, scenario="intersection")
        oc = ix_oracle_config(dh, cfg, E)
    else:
        oc = cfg = _abi.make_config(d, E, **kw)
    ended = np.asarray(fused["out/terminated"] | fused["out/truncated"], bool)
    stepped = np.concatenate([np.ones((1, E), bool), ~ended[:-1]])
    knife, hit = np.zeros((T, E), bool), np.zeros((T, E), bool)
    for t in range(T):
        st = {**_at(fused, "pre", t), **_at(fused, "pre_x", t)}
        with oracle.impact_margins(oc) as m:
            if ix:
                oracle_ix.step(oc, ix_oracle_state(st, cfg), acts[t])
            else:
                oracle.step(cfg, st, acts[t])
        margin = np.asarray(m.margin)
        knife[t] = stepped[t] & (margin.min(1) < KNIFE)
        hit[t] = stepped[t] & np.isfinite(margin).any(1)
    return knife, hit


def compare_fused_with_strict(fused: dict, strict: dict, knife, hit) -> dict:
    """Every step of the two runs, outside the env-steps of `knife` [T, E]: discrete planes EQUAL on every slot, floats within the
    one-step tolerances -- the pending impacts SIGNED (what is left after `knife` is well conditioned by the oracle's margin); the
    1e-6 of a collision step on the env-steps of `hit` [T, E].  Returns the largest differences per group."""
    T, E = knife.shape
    worst = {"state": 0.0, "state of collision steps": 0.0, "reward": 0.0, "obs": 0.0, "extras": 0.0}
    assert set(strict) == set(fused) | {"respawned"}
    np.testing.assert_array_equal(strict["actions"], fused["actions"])
    # teacher-forced: the strict run stepped from the fused run's states, and re-spawned the environments the fused run re-spawned
    done = fused["out/terminated"] | fused["out/truncated"]
    np.testing.assert_array_equal(strict["respawned"][0], np.zeros(E, bool))
    np.testing.assert_array_equal((strict["respawned"][1:] & ~knife[:-1]), (done[:-1] & ~knife[:-1]), err_msg="re-spawned environments")
    for k in fused:
        if k.startswith(("pre/", "pre_x/")):
            stepped = ~strict["respawned"]
            np.testing.assert_array_equal(strict[k][stepped], fused[k][stepped], err_msg=f"{k}: the strict run did not step from the recorded state")
    for t in range(T):
        keep = ~knife[t]
        what = f"step {t}"
        a, b = _at(fused, "post", t), _at(strict, "post", t)
        oa, ob = _at(fused, "out", t), _at(strict, "out", t)
        for k in ("terminated", "truncated", "crashed"):
            np.testing.assert_array_equal(ob[k][keep], oa[k][keep], err_msg=f"{what}: {k}")
        pres = (a["flags"] & _abi.F_ABSENT) == 0
        np.testing.assert_array_equal(((b["flags"] & _abi.F_ABSENT) == 0)[keep], pres[keep], err_msg=f"{what}: present")
        pres &= keep[:, None]
        for k in ("lane", "target_lane", "flags") + (("route",) if "route" in a else ()):
            np.testing.assert_array_equal(b[k][pres], a[k][pres], err_msg=f"{what}: {k}")
        ctrl = pres & ((a["flags"] & _abi.F_CONTROLLED) != 0)
        np.testing.assert_array_equal(b["speed_index"][ctrl], a["speed_index"][ctrl], err_msg=f"{what}: speed_index")
        if "road_steps" in a:
            np.testing.assert_array_equal(b["road_steps"][keep], a["road_steps"][keep], err_msg=f"{what}: road_steps")
        np.testing.assert_array_equal(b["time"][keep], a["time"][keep], err_msg=f"{what}: time")
        idm = pres & ((a["flags"] & (_abi.F_CONTROLLED | _abi.F_OBSTACLE)) == 0)
        collision = hit[t][:, None]   # (the vehicles of a collision step at 1e-6, every other env-step at 1e-7)
        for rows, atol, key in ((pres & ~collision, STATE_ATOL, "state"), (pres & collision, WRECK_ATOL, "state of collision steps")):
            for k in ("x", "y", "heading", "speed", "target_speed", "impact_x", "impact_y", "timer"):
                sel = rows & idm if k == "timer" else rows
                diff = np.abs(b[k][sel] - a[k][sel])
                worst[key] = max(worst[key], float(diff.max(initial=0)))
                assert diff.max(initial=0) <= atol, f"{what}: {k} differs by {diff.max():.3g} (> {atol})"
        for k in ("reward", "speed", "obs"):
            atol, key = {"reward": (REWARD_ATOL, "reward"), "speed": (STATE_ATOL, "state"), "obs": (OBS_ATOL, "obs")}[k]
            diff = np.abs(ob[k][keep].astype(np.float64) - oa[k][keep].astype(np.float64))
            worst[key] = max(worst[key], float(diff.max(initial=0)))
            assert diff.max(initial=0) <= atol, f"{what}: {k} differs by {diff.max():.3g} (> {atol})"
        xa, xb = _at(fused, "post_x", t), _at(strict, "post_x", t)
        for k in xa:
            diff = np.abs(xb[k][keep] - xa[k][keep])
            worst["extras"] = max(worst["extras"], float(diff.max(initial=0)))
            assert diff.max(initial=0) <= STATE_ATOL, f"{what}: {k} differs by {diff.max():.3g}"
    return worst


ROWS = strict_probe.rows()


@pytest.mark.parametrize("backend,label,d,kw,seed", _legs(ROWS, ident=lambda r: r[0].replace(" ", "-")))
def test_fused_against_strict(backend, label, d, kw, seed, tmp_path, request):
    """One row of tests/strict_probe.py: E = 32 environments, T = 6 policy steps, auto-reset on, episodes of 3 steps."""
    if backend == "hip":
        request.getfixturevalue("strict_lib")
    limit = 300 if backend == "emu" else 120   # (some ten times what a row takes)
    fused = _probe(backend, tmp_path / "fused.npz", "--row", label, strict=False, timeout=limit)
    strict = _probe(backend, tmp_path / "strict.npz", "--row", label, "--from", str(tmp_path / "fused.npz"), strict=True, timeout=limit)
    knife, hit = oracle_knife_edges(d, kw, fused)
    T, E = knife.shape
    assert (T, E) == (strict_probe.T, strict_probe.E)
    ended = int((fused["out/terminated"] | fused["out/truncated"]).sum())
    crashed = int(fused["out/crashed"].reshape(T, E, -1).any(2).sum())
    worst = compare_fused_with_strict(fused, strict, knife, hit)
    print(f"\nfused against strict [{backend}] {label}: {T * E} env-steps, {ended} episodes ended, {crashed} ended in a crash, "
          f"{int(hit.sum())} with a collision on the oracle, {int(knife.sum())} excluded as a push on the oracle's knife edge; "
          f"discrete planes equal on every slot; largest differences: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert ended >= E, "every environment ends an episode and is re-spawned inside the run"
    assert knife.sum() <= MAX_EXCLUDED * T * E, f"{int(knife.sum())} env-steps excluded"
    if not hit.any():
        assert not knife.any()


# --------------------------------------------------------------------------- 5. the fuzz families on the strict build

# (family, test of tests/test_fuzz_configs.py, chunk): the chunk numbers of tests/test_mutations.py -- chunk 1 of the intersection
# family holds a frame in which one vehicle is hit by two others, chunk 0 does not
FUZZ = [
    ("idm", "test_random_configurations_vs_oracle", 0),
    ("wide", "test_random_wide_configurations_vs_oracle", 0),
    ("linear", "test_random_linear_configurations_vs_oracle", 0),
    ("direct", "test_random_direct_configurations_vs_oracle", 0),
    ("lidar", "test_random_lidar_configurations_vs_oracle", 0),
    ("merge", "test_random_merge_configurations_vs_oracle", 0),
    ("intersection", "test_random_intersection_configurations_vs_oracle", 1),
]
LEDGER = re.compile(r"^(?:\w+ fuzz chunk \d+:|merge(?:-generic)? \[\w+\]:).*$", re.M)


def run_fuzz_chunk(backend: str, test: str, chunk: int, strict: bool, timeout: float):
    """One chunk of a fuzz family in a child (the fuzz tests are marked gpu and take their backend from HWY_FUZZ_BACKEND)."""
    env = {"HWY_FUZZ_BACKEND": backend, "HWY_FUZZ_FIRST": str(chunk), "HWY_FUZZ_CHUNKS": "1"}
    return strict_util.run_selection(backend, ["tests/test_fuzz_configs.py", "-k", test], strict=strict, extra_env=env, timeout=timeout,
                                     marker="gpu")


@pytest.mark.parametrize("backend,family,test,chunk", _legs(FUZZ))
def test_fuzz_chunk_on_the_strict_build(backend, family, test, chunk, request):
    """Under the existing ceilings (the assertions of the fuzz tests themselves).  What those tests print of tolerated and counted
    cases is printed again here: the strict column of the ledger in profiles/strict_arithmetic.md."""
    if backend == "hip":
        request.getfixturevalue("strict_lib")
    res = run_fuzz_chunk(backend, test, chunk, strict=True, timeout=1500 if backend == "emu" else 300)
    n = strict_util.assert_all_passed(res, f"{family} fuzz chunk {chunk} on the strict {backend} build")
    assert n == 1
    for line in LEDGER.findall(res.stdout) or ["(the family counts no tolerated case: it has none)"]:
        print(f"\nstrict ledger [{backend}] {family} chunk {chunk}: {line}")
