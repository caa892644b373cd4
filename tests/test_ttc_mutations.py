"""Load-bearing checks of the time-to-collision grid / finite-MDP planner kernel, by the method of tests/test_lidar_mutations.py:
a rule of the reference's ``compute_ttc_grid`` / ``transition_model`` / ``finite_mdp``, or a loop bound of the kernel, is broken in a
COPY of the kernel source (one text replacement in hwy_ttc.h), the CPU emulator (tests/emu/emu_ttc.cpp) is built from the copy, and
the tests of tests/test_ttc_parity.py that cover the rule must FAIL on it -- while they pass on the unmutated source:

* `sweep_first_pass_only`   -- the value sweep stops after its first 64 states: only ttc_states65 and ttc_max notice;
* `vehicles_first_pass_only` -- the vehicle loop stops after its first 64 slots (ttc_passes65 / ttc_passes130);
* `no_ceil`                 -- only int(ttc / tq) is marked, not int(ceil(ttc / tq));
* `store_not_max`           -- a cell takes the LAST cost, not the maximum (road 4 of ttc_crafted: the rear margin point comes after
  the centre point of the same cell);
* `no_equal_speed_skip`     -- `ego_speed == other.speed` is not skipped.  Road 0 of ttc_crafted does NOT catch it (the candidate it
  skips lies 30 m / not_zero(0) = 3000 s away); this mutant survived every fixture until road 10 was added;
* `not_zero_always_plus`    -- utils.not_zero gives +eps for every small value (road 1);
* `dot_without_sine`        -- np.dot(other.direction, vehicle.direction) loses its sine term (road 8; on road 6 the observer's
  heading is 0, so the term is 0 there);
* `speed_at_every_time`     -- FASTER / SLOWER change the speed index at every j, not only at j == 0;
* `terminal_without_collision` -- `terminal` is the end of the horizon only;
* `argmax_last`             -- the action is the LAST maximum of the Q row (numpy's argmax is the first);
* `small_class_off_by_one`  -- the sweep reads its cell at s * T + j + (s >= 64): an index rule that is right in the first pass only.

Each case runs the real test functions in a subprocess with HWY_EMU_TTC_LIB pointing at the mutant."""
import pytest

from tests import mutation_util

H = "hwy_ttc.h"
MUTANTS = {
    "sweep_first_pass_only": [(H, "for (int s = lane; s < states; s += 64) {", "for (int s = lane; s < states && s < 64; s += 64) {")],
    "vehicles_first_pass_only": [(H, "for (int base = 0; base < p.N; base += 64) {", "for (int base = 0; base < p.N && base < 64; base += 64) {")],
    "no_ceil": [(H, "if (up < horizon_steps) ttc_mark(sh_cell, cell0 + (int)up, code);", "(void)up;")],
    "store_not_max": [(H, "__hip_atomic_fetch_max(&cells[index], code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);",
                       "__hip_atomic_store(&cells[index], code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);")],
    "no_equal_speed_skip": [(H, "if (ego_speed == ospeed) continue;", "if (false && ego_speed == ospeed) continue;")],
    "not_zero_always_plus": [(H, "return x >= 0 ? eps : -eps;", "return eps;")],
    "dot_without_sine": [(H, "const double dot = d0 + d1;", "const double dot = d0 + 0 * d1;")],
    "speed_at_every_time": [(H, "const int hf = (j == 0 && h < V - 1) ? h + 1 : h, hs = (j == 0 && h > 0) ? h - 1 : h;",
                             "const int hf = (h < V - 1) ? h + 1 : h, hs = (h > 0) ? h - 1 : h;")],
    "terminal_without_collision": [(H, "const bool terminal = code == 2 || j == T - 1;", "const bool terminal = j == T - 1;")],
    "argmax_last": [(H, "if (k == 0 || qa[k] > best) { best = qa[k]; arg = k; }", "if (k == 0 || qa[k] >= best) { best = qa[k]; arg = k; }")],
    "small_class_off_by_one": [(H, "const int32_t code = sh_cell[s * T + j];", "const int32_t code = sh_cell[s * T + j + (s >= 64 && j + 1 < T)];")],
}
PARITY = ["tests/test_ttc_parity.py", "-m", "not gpu"]
NEW = "ttc_states65 or ttc_max"                                  # the fixtures that hold the second pass of the sweep
BEFORE = "not (ttc_cells1024 or ttc_cells1025 or ttc_states64 or ttc_states65 or ttc_max)"   # everything recorded before them
CASES = [
    ("sweep_first_pass_only", PARITY + ["-k", f"planner and ({NEW})"]),
    ("vehicles_first_pass_only", PARITY + ["-k", "fixture_grids and (ttc_passes65 or ttc_passes130)"]),
    ("no_ceil", PARITY + ["-k", "fixture_grids and (ttc_fast or ttc_crafted)"]),
    ("store_not_max", PARITY + ["-k", "fixture_grids and ttc_crafted"]),
    ("no_equal_speed_skip", PARITY + ["-k", "fixture_grids and ttc_crafted"]),
    ("not_zero_always_plus", PARITY + ["-k", "fixture_grids and ttc_crafted"]),
    ("dot_without_sine", PARITY + ["-k", "fixture_grids and ttc_crafted"]),
    ("speed_at_every_time", PARITY + ["-k", "planner and (ttc_fast or ttc_speeds8)"]),
    ("terminal_without_collision", PARITY + ["-k", "planner and (ttc_fast or ttc_crash)"]),
    ("argmax_last", PARITY + ["-k", "planner and (ttc_lanes1 or ttc_horizon1)"]),
    ("small_class_off_by_one", PARITY + ["-k", f"planner and ({NEW})"]),
]


def build_mutant(name: str) -> str:
    return mutation_util.build_mutant(MUTANTS[name], "emu_ttc.cpp", f"libhwy_emu_ttc_mut_{name}.so")


def run_selection(lib, selection):
    return mutation_util.run_selection(lib, selection, "HWY_EMU_TTC_LIB")


def _build_the_suites_own():
    from tests.emu import emu
    emu.build_all()  # (before two processes could both start one)


@pytest.mark.parametrize("mutant,selection", CASES, ids=[c[0] for c in CASES])
def test_broken_rule_fails_the_comparison_that_covers_it(mutant, selection):
    from concurrent.futures import ThreadPoolExecutor
    _build_the_suites_own()
    with ThreadPoolExecutor(2) as pool:   # the control and the mutant side by side (two subprocesses)
        f_good = pool.submit(run_selection, None, selection)
        f_bad = pool.submit(lambda: run_selection(build_mutant(mutant), selection))
        good, bad = f_good.result(), f_bad.result()
    assert good.returncode == 0 and " passed" in good.stdout, f"the selection must pass on the unmutated kernel source:\n{good.stdout[-3000:]}"
    assert bad.returncode == 1 and "AssertionError" in bad.stdout, \
        f"mutant {mutant} SURVIVED {selection} (rc {bad.returncode}):\n{bad.stdout[-3000:]}"


@pytest.mark.parametrize("mutant", ["sweep_first_pass_only", "small_class_off_by_one"])
def test_second_pass_of_the_sweep_rests_on_the_new_fixtures_alone(mutant):
    """A planner whose second pass is missing or wrong passes EVERYTHING recorded before ttc_states65 / ttc_max (no fixture before
    them has more than 48 states), and fails each of the two on its own."""
    _build_the_suites_own()
    lib = build_mutant(mutant)
    before = run_selection(lib, PARITY + ["-k", BEFORE])
    assert before.returncode == 0 and " passed" in before.stdout, f"mutant {mutant} fails a fixture without a second pass:\n{before.stdout[-3000:]}"
    for name in ("ttc_states65", "ttc_max"):
        bad = run_selection(lib, PARITY + ["-k", f"planner and {name}"])
        assert bad.returncode == 1 and "AssertionError" in bad.stdout, f"mutant {mutant} SURVIVED {name}:\n{bad.stdout[-3000:]}"


@pytest.mark.parametrize("road,mutant", [(10, "no_equal_speed_skip"), (1, "not_zero_always_plus"), (4, "store_not_max"),
                                         (8, "dot_without_sine")])
def test_crafted_road_catches_its_rule(road, mutant):
    """Each hand-placed road of ttc_crafted is what its rule rests on: the mutant's grid of THAT road differs from the reference's."""
    import numpy as np

    from tests.ttc_util import TtcGolden
    g = TtcGolden("ttc_crafted")
    done = mutation_util.run_selection(build_mutant(mutant), ["tests/test_ttc_mutations.py", "-k", "print_crafted_grid", "-s"],
                                       "HWY_EMU_TTC_LIB", env_extra={"HWY_TTC_MUTANT_ROAD": str(road)})
    assert done.returncode == 0, done.stdout[-3000:]
    line = next(ln for ln in done.stdout.splitlines() if ln.startswith("GRID "))
    got = np.array([float(v) for v in line.split()[1:]]).reshape(g.get("grid")[road, 0].shape)
    assert (got != g.get("grid")[road, 0]).any(), f"mutant {mutant} gives the reference's grid on road {road}"


def test_print_crafted_grid():
    """Helper of test_crafted_road_catches_its_rule (run in its subprocess, on the mutant): prints the emulation's grid of one road
    of ttc_crafted; on its own it only checks the grid's values."""
    import os

    import numpy as np

    from tests.ttc_util import TtcGolden, make_engine
    road = int(os.environ.get("HWY_TTC_MUTANT_ROAD", "0"))
    g = TtcGolden("ttc_crafted")
    eng = make_engine("emu", g.hwy_config())
    g.load(eng)
    grid = eng.ttc_grid(g.params())[road, 0]
    assert np.isin(grid, (0.0, 0.5, 1.0)).all()
    print("GRID " + " ".join(str(float(v)) for v in grid.ravel()))
