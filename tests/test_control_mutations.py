"""Load-bearing checks of the direct-ego-control kernels, by the method of tests/test_mutations.py: a rule of the reference is
broken in a COPY of the kernel source (one text replacement per file), the CPU emulator (tests/emu/emu_control.cpp) is built from
the copy, and the test of tests/test_control_parity.py that covers the rule must FAIL on it -- while it passes on the unmutated
source:

* `fused_speed_update`   -- the ego's speed += a * dt as ONE fused multiply-add: the last bit of the speed differs from the
  reference's product-then-sum, and next to +-MAX_SPEED that bit picks the branch of clip_actions (direct_brake);
* `clip_not_sticky`      -- clip_actions clips a copy: the stored acceleration is the action's again on the next frame, where the
  reference keeps what the clip wrote for the rest of the policy step (direct_throttle);
* `ego_is_abort_rival`   -- the plain-Vehicle ego counts as a rival in the lane-change abort rule, with the target lane its slot
  shows (behavior.py:237 skips it: isinstance(v, ControlledVehicle));
* `ego_follower_target_is_its_speed` -- a MOBIL caller reads the ego's own speed as its target speed instead of
  getattr(ego, "target_speed", 0) = 0: cut-ins in front of a moving ego become safe;
* `reward_from_target_lane` -- the right-lane reward reads the ego's target-lane slot (last step's lane) instead of its lane.

Each case runs the real test functions in a subprocess with HWY_EMU_CONTROL_LIB pointing at the mutant."""
import pytest

from tests import mutation_util

RIVAL = ("const bool rival = !(EG::DIRECT && controlled);", "const bool rival = true;")
MUTANTS = {
    "fused_speed_update": [("hwy_device.h", "  const double dv = accel * dt;\n  return v + dv;", "  return v + accel * dt;")],
    "clip_not_sticky": [("hwy_device.h", "  stored = c;  // (sticky: the vehicle keeps what the clip wrote)", "  (void)stored;")],
    "ego_is_abort_rival": [("hwy_device.h",) + RIVAL, ("hwy_wave.h",) + RIVAL],
    "ego_follower_target_is_its_speed": [("hwy_device.h", "  (void)v;\n  return 0.0;", "  return v;")],
    "reward_from_target_lane": [("hwy_device.h", "return EG::DIRECT ? me.lane : me.tgt;", "return me.tgt;")],
}
PARITY = ["tests/test_control_parity.py", "-m", "not gpu"]
CASES = [
    ("fused_speed_update", PARITY + ["-k", "direct_brake or brake_run"]),
    ("clip_not_sticky", PARITY + ["-k", "direct_throttle and (teacher_forced or free_running)"]),
    ("ego_is_abort_rival", PARITY + ["-k", "free_running and direct_rival"]),
    ("ego_follower_target_is_its_speed", PARITY + ["-k", "free_running and (direct_v0 or direct_k5)"]),
    ("reward_from_target_lane", PARITY + ["-k", "free_running and direct_crash_many"]),
]


def build_mutant(name: str) -> str:
    return mutation_util.build_mutant(MUTANTS[name], "emu_control.cpp", f"libhwy_emu_control_mut_{name}.so")


def run_selection(lib, selection):
    return mutation_util.run_selection(lib, selection, "HWY_EMU_CONTROL_LIB")


@pytest.mark.parametrize("mutant,selection", CASES, ids=[c[0] for c in CASES])
def test_broken_rule_fails_the_comparison_that_covers_it(mutant, selection):
    from concurrent.futures import ThreadPoolExecutor
    from tests.emu import emu
    emu.build("control")   # (the suite's own emulator build, before two processes could both start building it)
    with ThreadPoolExecutor(2) as pool:   # the control and the mutant side by side (two subprocesses)
        f_good = pool.submit(run_selection, None, selection)
        f_bad = pool.submit(lambda: run_selection(build_mutant(mutant), selection))
        good, bad = f_good.result(), f_bad.result()
    assert good.returncode == 0 and " passed" in good.stdout, f"the selection must pass on the unmutated kernel source:\n{good.stdout[-3000:]}"
    assert bad.returncode == 1 and "AssertionError" in bad.stdout, \
        f"mutant {mutant} SURVIVED {selection} (rc {bad.returncode}):\n{bad.stdout[-3000:]}"
