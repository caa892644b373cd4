"""Load-bearing checks of the LidarObservation kernel, by the method of tests/test_mutations.py: a rule of the reference's
``trace()`` is broken in a COPY of the kernel source (one text replacement in hwy_lidar.h), the CPU emulator
(tests/emu/emu_lidar.cpp) is built from the copy, and the tests of tests/test_lidar_parity.py that cover the rule must FAIL on it
-- while they pass on the unmutated source:

* `le_to_lt`            -- a candidate is taken when its distance is < the stored one: the EARLIER obstacle wins a tie;
* `fold_in_f64`         -- the grid is f64 while it is folded and rounded at the end: a candidate between the stored distance and
  its float32 rounding is taken;
* `no_pi_wrap`          -- the +-pi wrap of the sector is dropped: an obstacle straight behind covers every cell but its own;
* `width_not_subtracted` -- the centre candidate is the centre distance itself, not minus WIDTH / 2;
* `absolute_velocity`   -- the observer's velocity is not subtracted;
* `range_on_corners`    -- the range test looks at the nearest corner instead of the centre.

Each case runs the real test functions in a subprocess with HWY_EMU_LIDAR_LIB pointing at the mutant."""
import pytest

from tests import mutation_util

NEAREST_CORNER = ("fmin(fmin(lidar_norm2(cx[0] - ox, cy[0] - oy), lidar_norm2(cx[1] - ox, cy[1] - oy)), "
                  "fmin(lidar_norm2(cx[2] - ox, cy[2] - oy), lidar_norm2(cx[3] - ox, cy[3] - oy)))")
MUTANTS = {
    "le_to_lt": [("hwy_lidar.h", "  if (distance <= (double)gd) {", "  if (distance < (double)gd) {")],
    "fold_in_f64": [("hwy_lidar.h", "typedef float lidar_cell_t;", "typedef double lidar_cell_t;")],
    "no_pi_wrap": [("hwy_lidar.h", "if (min_angle < -HWY_PI / 2 && HWY_PI / 2 < max_angle) {", "if (false && min_angle < max_angle) {")],
    "width_not_subtracted": [("hwy_lidar.h", "const double distance = center_distance - HWY_VEH_WIDTH / 2;",
                              "const double distance = center_distance;")],
    "absolute_velocity": [("hwy_lidar.h", "const double rvx = vx - ovx, rvy = vy - ovy;", "const double rvx = vx + 0 * ovx, rvy = vy + 0 * ovy;")],
    "range_on_corners": [("hwy_lidar.h", "const bool in_range = !(center_distance > R);", f"const bool in_range = !({NEAREST_CORNER} > R);")],
}
PARITY = ["tests/test_lidar_parity.py", "-m", "not gpu"]
CASES = [
    ("le_to_lt", PARITY + ["-k", "crafted"]),
    ("fold_in_f64", PARITY + ["-k", "crafted"]),
    ("no_pi_wrap", PARITY + ["-k", "crafted or (recorded_states and lidar_fast)"]),
    ("width_not_subtracted", PARITY + ["-k", "crafted or (recorded_states and lidar_crash)"]),
    ("absolute_velocity", PARITY + ["-k", "crafted or (free_running and lidar_fast)"]),
    ("range_on_corners", PARITY + ["-k", "crafted or (recorded_states and lidar_cells64_raw)"]),
]


def build_mutant(name: str) -> str:
    return mutation_util.build_mutant(MUTANTS[name], "emu_lidar.cpp", f"libhwy_emu_lidar_mut_{name}.so")


def run_selection(lib, selection):
    return mutation_util.run_selection(lib, selection, "HWY_EMU_LIDAR_LIB")


@pytest.mark.parametrize("mutant,selection", CASES, ids=[c[0] for c in CASES])
def test_broken_rule_fails_the_comparison_that_covers_it(mutant, selection):
    from concurrent.futures import ThreadPoolExecutor
    from tests.emu import emu
    emu.build_all()  # (the suite's own emulator builds, before two processes could both start one)
    with ThreadPoolExecutor(2) as pool:   # the control and the mutant side by side (two subprocesses)
        f_good = pool.submit(run_selection, None, selection)
        f_bad = pool.submit(lambda: run_selection(build_mutant(mutant), selection))
        good, bad = f_good.result(), f_bad.result()
    assert good.returncode == 0 and " passed" in good.stdout, f"the selection must pass on the unmutated kernel source:\n{good.stdout[-3000:]}"
    assert bad.returncode == 1 and "AssertionError" in bad.stdout, \
        f"mutant {mutant} SURVIVED {selection} (rc {bad.returncode}):\n{bad.stdout[-3000:]}"


@pytest.mark.parametrize("mutant", ["le_to_lt", "fold_in_f64", "range_on_corners", "no_pi_wrap"])
def test_crafted_roads_alone_catch_the_fold_and_range_rules(mutant):
    """The hand-placed roads are what these four rules rest on: the bit-for-bit test alone fails on each."""
    bad = run_selection(build_mutant(mutant), PARITY + ["-k", "crafted_roads_bit_for_bit"])
    assert bad.returncode == 1 and "AssertionError" in bad.stdout, f"mutant {mutant} SURVIVED lidar_crafted:\n{bad.stdout[-3000:]}"
