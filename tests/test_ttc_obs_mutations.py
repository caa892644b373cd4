"""Load-bearing checks of the TimeToCollision observation kernel, by the method of tests/test_ttc_mutations.py: a rule of the
reference's ``TimeToCollisionObservation.observe`` is broken in a COPY of the kernel source (one text replacement in
hwy_collision_obs.h), the CPU emulator (tests/emu/emu_ttc_obs.cpp) is built from the copy, and the tests of
tests/test_ttc_obs_parity.py that cover the rule must FAIL on it -- while they pass on the unmutated source:

* `speed_padding_of_ones` -- a speed index outside the ladder gives a row of ones, like a lane off the road, instead of the
  repeated first / last row (np.repeat, observation.py:141-143);
* `lane_padding_of_zeros` -- a lane off the road gives zeros instead of ones (observation.py:133-134);
* `no_ceil`               -- only int(ttc / tq) is marked, not int(ceil(ttc / tq)).

Each case runs the real test functions in a subprocess with HWY_EMU_TTC_OBS_LIB pointing at the mutant."""
import pytest

from tests import mutation_util

H = "hwy_collision_obs.h"
MUTANTS = {
    "speed_padding_of_ones": [(H, "sh_cell[k] = (wl >= 0 && wl < L) ? 0 : 2;",
                               "const int wv = word_speed_index(wme) + k / (HWY_COLLISION_OBS_SIDE * T) - 1; "
                               "sh_cell[k] = (wl >= 0 && wl < L && wv >= 0 && wv < V) ? 0 : 2;")],
    "lane_padding_of_zeros": [(H, "sh_cell[k] = (wl >= 0 && wl < L) ? 0 : 2;", "sh_cell[k] = (wl >= 0 && wl < L) ? 0 : 0;")],
    "no_ceil": [(H, "if (up < horizon_steps) ttc_mark(sh_cell, cell0 + (int)up, code);", "(void)up;")],
}
PARITY = ["tests/test_ttc_obs_parity.py", "-m", "not gpu"]
CASES = [
    ("speed_padding_of_ones", PARITY + ["-k", "fixture_observations and (ttcobs_ladder or ttcobs_speeds2)"]),
    ("speed_padding_of_ones", PARITY + ["-k", "window_of_the_recorded_reference_grid and ttc_speeds2"]),
    ("lane_padding_of_zeros", PARITY + ["-k", "fixture_observations and (ttcobs_lanes1 or ttcobs_edges)"]),
    ("no_ceil", PARITY + ["-k", "fixture_observations and (ttcobs_fast or ttcobs_pf5)"]),
    ("no_ceil", PARITY + ["-k", "own_states and fast"]),
]


def build_mutant(name: str) -> str:
    from tests.emu import emu_ttc_obs  # noqa: F401  (registers the unit)
    return mutation_util.build_mutant(MUTANTS[name], "emu_ttc_obs.cpp", f"libhwy_emu_ttc_obs_mut_{name}.so")


@pytest.mark.parametrize("mutant,selection", CASES, ids=[f"{c[0]}-{k}" for k, c in enumerate(CASES)])
def test_broken_rule_fails_the_comparison_that_covers_it(mutant, selection):
    from concurrent.futures import ThreadPoolExecutor

    from tests.emu import emu, emu_ttc_obs  # noqa: F401
    emu.build_all()  # (before two processes could both start one)
    with ThreadPoolExecutor(2) as pool:   # the control and the mutant side by side (two subprocesses)
        f_good = pool.submit(mutation_util.run_selection, None, selection, "HWY_EMU_TTC_OBS_LIB")
        f_bad = pool.submit(lambda: mutation_util.run_selection(build_mutant(mutant), selection, "HWY_EMU_TTC_OBS_LIB"))
        good, bad = f_good.result(), f_bad.result()
    assert good.returncode == 0 and " passed" in good.stdout, f"the selection must pass on the unmutated kernel source:\n{good.stdout[-3000:]}"
    assert bad.returncode == 1 and "AssertionError" in bad.stdout, \
        f"mutant {mutant} SURVIVED {selection} (rc {bad.returncode}):\n{bad.stdout[-3000:]}"
