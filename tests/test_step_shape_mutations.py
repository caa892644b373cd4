"""Seeded bugs in the step kernels compiled for the registered configurations (csrc/hwy_wave.h: FixedShape; hwy_launch_family.h:
launch_step_shape), as tests/test_mutations.py seeds them elsewhere: the CPU emulator is built from a mutated COPY of the kernel
source and the comparison that covers the mutated code runs against it in a subprocess -- it must FAIL there and pass on the
unmutated build.

* `shape_full_scan_negated` -- a shape derives FULL_SCAN from its flags; the negation is lost, so highway-v0's shape (V0Shape4) is
  built WITHOUT the full pairwise window scan and the two fast shapes with it.  This mutant SURVIVES, and must: FULL_SCAN selects
  a faster path, not a rule -- without it every checker goes through the checker loop, "correct for any set of checkers"
  (hwy_wave.h, above wave_policy_step), and with it the scan only runs when every vehicle checks (all_check).  The test below
  records that, so that the day FULL_SCAN starts to decide a result the record fails;
* `shape_ego_only_collisions` -- the same lost negation in a kernel whose build without the scan checks the ego alone (the
  nearest site at which the bug the negation stands for -- highway-v0's shape misses what its traffic hits -- changes a result:
  the ballot of the checkers).  The ORACLE comparison under auto-reset (tests/test_step_shapes_oracle.py) must fail on it for
  V0Shape4, through the collision between two vehicles of the traffic its seeds were chosen for;
* `shape_launch_swapped`    -- launch_step_shape launches highway-v0's case with the kernel of highway-fast-v0 on 4 lanes.  On the
  device that kernel would ASSUME 5 frames per step and ego-only collisions; the emulation checks what the device build assumes
  (HWY_SHAPE_FIXED traps), so the run dies instead of computing something."""
import pytest

from tests import mutation_util

MUTANTS = {
    "shape_full_scan_negated": [
        ("hwy_wave.h", "static constexpr bool FULL_SCAN = !(FLAGS_ & HWY_C_EGO_ONLY_COLLISIONS);",
         "static constexpr bool FULL_SCAN = (FLAGS_ & HWY_C_EGO_ONLY_COLLISIONS);")],
    "shape_ego_only_collisions": [
        ("hwy_wave.h", "static constexpr bool FULL_SCAN = !(FLAGS_ & HWY_C_EGO_ONLY_COLLISIONS);",
         "static constexpr bool FULL_SCAN = (FLAGS_ & HWY_C_EGO_ONLY_COLLISIONS);"),
        ("hwy_wave.h", "const u64 chk = __ballot(active && i_check);", "const u64 chk = __ballot(active && i_check && (FULL_SCAN || controlled));")],
    "shape_launch_swapped": [
        ("hwy_launch_family.h", "case V0Shape4::ID: return B::launch(hwy_shape_wave_kernel<V0Shape4, WPE>",
         "case V0Shape4::ID: return B::launch(hwy_shape_wave_kernel<FastShape4, WPE>")],
}
# (mutant, pytest selection, how the mutant's run must end: "assertion" = pytest reports a failed comparison, "died" = the kernel's
# own check trapped and took the process with it)
ORACLE_V0 = ["tests/test_step_shapes_oracle.py", "-m", "not gpu", "-k", "emu-v0-4"]
CASES = [
    ("shape_ego_only_collisions", ORACLE_V0, "assertion"),
    ("shape_launch_swapped", ["tests/test_step_shapes.py", "-m", "not gpu", "-k", "test_the_registered_configurations_report_their_shape and v0"],
     "died"),
]


def run_selection(lib, selection):
    return mutation_util.run_selection(lib, selection, "HWY_EMU_LIB")


def build_mutant(name: str) -> str:
    return mutation_util.build_mutant(MUTANTS[name], "emu_engine.cpp", f"libhwy_emu_mut_{name}.so")


@pytest.mark.parametrize("mutant,selection,end", CASES, ids=[c[0] for c in CASES])
def test_seeded_shape_bug_fails_the_test_that_covers_it(mutant, selection, end):
    from concurrent.futures import ThreadPoolExecutor
    from tests.emu import emu
    emu.build()   # (the suite's own emulator build, before two processes could both start building it)
    with ThreadPoolExecutor(2) as pool:   # the control and the mutant side by side (two subprocesses)
        f_good = pool.submit(run_selection, None, selection)
        f_bad = pool.submit(lambda: run_selection(build_mutant(mutant), selection))
        good, bad = f_good.result(), f_bad.result()
    assert good.returncode == 0 and " passed" in good.stdout, f"the selection must pass on the unmutated kernel source:\n{good.stdout[-3000:]}"
    if end == "assertion":
        assert bad.returncode == 1 and "AssertionError" in bad.stdout, \
            f"mutant {mutant} SURVIVED {selection} (rc {bad.returncode}):\n{bad.stdout[-3000:]}"
    else:   # a trap is a signal: the child never gets to print a summary, let alone a pass
        assert bad.returncode not in (0, 1, 5) and " passed" not in bad.stdout, \
            f"mutant {mutant}: expected the kernel's own check to end the run (rc {bad.returncode}):\n{bad.stdout[-3000:]}"


def test_the_negated_full_scan_alone_changes_no_result():
    """`shape_full_scan_negated` passes the oracle comparison AND bit-identity with the generic kernel at every size: the kernel
    without the window scan is the same function (see the module docstring)."""
    from tests.emu import emu
    emu.build()
    lib = build_mutant("shape_full_scan_negated")
    for selection in (ORACLE_V0, ["tests/test_step_shapes.py", "-m", "not gpu", "-k", "test_shape_kernel_equals_generic_kernel"]):
        res = run_selection(lib, selection)
        assert res.returncode == 0 and " passed" in res.stdout, \
            f"FULL_SCAN decides a result now: {selection} (rc {res.returncode}):\n{res.stdout[-3000:]}"
