"""The oracle fuzz of the Linear, direct-control and Lidar families bites: by the method of tests/test_mutations.py (one text
replacement per file in a COPY of the kernel source, the CPU emulator built from the copy), three chunks of a family's fuzz
(tests/test_fuzz_configs.py, HWY_FUZZ_BACKEND=emu; for the last mutant an edge case) must FAIL on the mutant while they pass on
the unmutated source.

* `linear_class_gain_lost_beyond_one_wavefront` -- the workgroup kernel with two or more wavefronts (N > 64) tests the lane-change
  incentive against IDMVehicle's 0.2 instead of the traffic class's LANE_CHANGE_MIN_ACC_GAIN (1.0 for Aggressive / Defensive).
  The committed fixtures do NOT kill it: their Aggressive / Defensive roads hold 31 and 32 vehicles, the one fixture beyond 64
  (linear_n100) is LinearVehicle traffic, whose gain IS 0.2.
* `direct_steering_index_is_the_quotient` -- the steering index of a DiscreteAction id taken as id / n_steer instead of the
  remainder.  The committed fixtures kill it too (every fixture of tests/golden/control with a steered axis).
* `lidar_wrap_sector_and` -- the sector of an obstacle whose corners wrap around cell 0 taken as `lane >= start && lane <= end`.
  The committed fixtures kill it too (tests/test_lidar_parity.py: the leader straight ahead of every recorded road).
* `lidar_third_pass_dropped` -- the Lidar kernel stops after two passes of 64 obstacles: vehicles 128 .. 255 are never traced.
  The committed fixtures do NOT kill it (the largest Lidar fixture, lidar_n100, holds 101 vehicles), and neither do three chunks of
  the fuzz: only an observer in the back half of a road of more than 128 vehicles has such obstacles in range.  The edge case
  built for it does (tests/test_families_edge_cases.py: test_lidar_every_obstacle_pass_reaches_an_observer), same method.

What the fixtures do with each mutant was established by running tests/test_traffic_parity.py, tests/test_control_parity.py and
tests/test_lidar_parity.py (-m "not gpu") against the same mutant libraries."""
import pytest

from tests import mutation_util

STEER_OLD = "is = acted ? {0} - ia * da->n_steer : 0;"
STEER_NEW = "is = acted ? ({0} / da->n_steer) % da->n_steer : 0;"
MUTANTS = {
    "linear_class_gain_lost_beyond_one_wavefront": ("emu_traffic.cpp", "HWY_EMU_TRAFFIC_LIB", "linear", [
        ("hwy_device.h", "if (jerk < (TM::LINEAR ? la.lc_gain : HWY_LC_MIN_ACC_GAIN)) continue;",
         "if (jerk < (TM::LINEAR && NW < 2 ? la.lc_gain : HWY_LC_MIN_ACC_GAIN)) continue;")]),
    "direct_steering_index_is_the_quotient": ("emu_control.cpp", "HWY_EMU_CONTROL_LIB", "direct", [
        ("hwy_device.h", STEER_OLD.format("id"), STEER_NEW.format("id")), ("hwy_wave.h", STEER_OLD.format("act0"), STEER_NEW.format("act0"))]),
    "lidar_wrap_sector_and": ("emu_lidar.cpp", "HWY_EMU_LIDAR_LIB", "lidar", [
        ("hwy_lidar.h", "(lane >= start || lane <= end);", "(lane >= start && lane <= end);")]),
    "lidar_third_pass_dropped": ("emu_lidar.cpp", "HWY_EMU_LIDAR_LIB", "edge:every_obstacle_pass", [
        ("hwy_lidar.h", "for (int base = 0; base < p.N; base += 64) {", "for (int base = 0; base < p.N && base < 128; base += 64) {")]),
}
FUZZ_ENV = {"HWY_FUZZ_BACKEND": "emu", "HWY_FUZZ_FIRST": "0", "HWY_FUZZ_CHUNKS": "3"}


def selection(family):
    if family.startswith("edge:"):
        return ["tests/test_families_edge_cases.py", "-m", "not gpu", "-k", family[5:]]
    return ["tests/test_fuzz_configs.py", "-m", "gpu", "-k", f"test_random_{family}_configurations_vs_oracle"]


def build_mutant(name: str) -> str:
    driver, _, _, sites = MUTANTS[name]
    return mutation_util.build_mutant(sites, driver, f"libhwy_emu_families_mut_{name}.so")


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_the_oracle_fuzz_alone_kills_the_mutant(mutant):
    from concurrent.futures import ThreadPoolExecutor
    from tests.emu import emu
    emu.build_all()  # (the suite's own emulator builds, before two processes could both start one)
    _, env_var, family, _ = MUTANTS[mutant]
    with ThreadPoolExecutor(2) as pool:   # the control and the mutant side by side (two subprocesses)
        f_good = pool.submit(mutation_util.run_selection, None, selection(family), env_var, FUZZ_ENV)
        f_bad = pool.submit(lambda: mutation_util.run_selection(build_mutant(mutant), selection(family), env_var, FUZZ_ENV))
        good, bad = f_good.result(), f_bad.result()
    n = "1 passed" if family.startswith("edge:") else "3 passed"
    assert good.returncode == 0 and n in good.stdout, f"the selection must pass on the unmutated kernel source:\n{good.stdout[-3000:]}"
    assert bad.returncode == 1 and "AssertionError" in bad.stdout, f"mutant {mutant} SURVIVED {selection(family)} (rc {bad.returncode}):\n{bad.stdout[-3000:]}"
