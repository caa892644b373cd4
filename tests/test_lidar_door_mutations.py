"""Load-bearing checks of the Lidar door's kernel, by the method of tests/test_lidar_mutations.py: what generalises the highway
kernel is broken in a COPY of the kernel source (one text replacement in hwy_lidar_door.h), the CPU emulator
(tests/emu/emu_lidar_door.cpp) is built from the copy, and the tests of tests/test_lidar_door_parity.py that cover the rule must
FAIL on it -- while they pass on the unmutated source:

* `obstacle_with_a_vehicles_length` -- the merge scenarios' Obstacle traced as 5 m x 2 m instead of 2 m x 2 m;
* `ix_observer_from_agent_index`    -- the intersection's observer taken from agent_index[a] instead of the a-th controlled slot;
* `absent_slots_traced`             -- slots with HWY_F_ABSENT traced like vehicles.

Each case runs the real test functions in a subprocess with HWY_EMU_LIDAR_DOOR_LIB pointing at the mutant."""
import pytest

from tests import mutation_util

H = "hwy_lidar_door.h"
ENV = "HWY_EMU_LIDAR_DOOR_LIB"
MUTANTS = {
    "obstacle_with_a_vehicles_length": [(H, "((flags & HWY_F_OBSTACLE) ? HWY_OBSTACLE_LENGTH : HWY_VEH_LENGTH) / 2", "HWY_VEH_LENGTH / 2")],
    "ix_observer_from_agent_index": [(H, "if (ix) {  // the a-th present slot", "if (ix && p.N < 0) {  // the a-th present slot")],
    "absent_slots_traced": [(H, "j != me && !(flags & HWY_F_ABSENT)) {", "j != me) {")],
}
PARITY = ["tests/test_lidar_door_parity.py", "-m", "not gpu", "-k"]
CASES = [
    ("obstacle_with_a_vehicles_length", PARITY + ["every_recorded_state and door_crafted"]),
    ("obstacle_with_a_vehicles_length", PARITY + ["every_recorded_state and door_merge_v1"]),
    ("ix_observer_from_agent_index", PARITY + ["every_recorded_state and door_ix-"]),
    ("ix_observer_from_agent_index", PARITY + ["every_recorded_state and door_ix_ma3"]),
    ("absent_slots_traced", PARITY + ["every_recorded_state and door_crafted"]),
]


def build_mutant(name: str) -> str:
    from tests.emu import emu_lidar_door  # noqa: F401  (registers the unit)
    return mutation_util.build_mutant(MUTANTS[name], "emu_lidar_door.cpp", f"libhwy_emu_lidar_door_mut_{name}.so")


@pytest.mark.parametrize("mutant,selection", CASES, ids=[f"{c[0]}-{k}" for k, c in enumerate(CASES)])
def test_broken_rule_fails_the_comparison_that_covers_it(mutant, selection):
    from concurrent.futures import ThreadPoolExecutor

    from tests.emu import emu, emu_lidar_door  # noqa: F401
    emu.build_all()  # (before two processes could both start one)
    with ThreadPoolExecutor(2) as pool:   # the control and the mutant side by side (two subprocesses)
        f_good = pool.submit(mutation_util.run_selection, None, selection, ENV)
        f_bad = pool.submit(lambda: mutation_util.run_selection(build_mutant(mutant), selection, ENV))
        good, bad = f_good.result(), f_bad.result()
    assert good.returncode == 0 and " passed" in good.stdout, f"the selection must pass on the unmutated kernel source:\n{good.stdout[-3000:]}"
    assert bad.returncode == 1 and "AssertionError" in bad.stdout, \
        f"mutant {mutant} SURVIVED {selection} (rc {bad.returncode}):\n{bad.stdout[-3000:]}"
