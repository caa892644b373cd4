"""tests/test_spawn_paths.py bites: by the method of tests/test_mutations.py (one text replacement in a COPY of the kernel source,
the CPU emulator built from the copy), each mutant of a device spawn must FAIL a named row of the table while that row passes on
the unmutated source.

* `draw_index_wraps_at_64` -- spawn_draw keys the lane / speed draw with `vi & 63`: vehicle 64 + k repeats the draws of vehicle k.
  Every spawn beyond one wavefront is wrong, and consistently so in every kernel built from spawn_draw.
* `workgroup_linear_respawn_draws_episode_0` -- the workgroup kernel's re-spawn draws the Linear parameters on episode 0's stream
  instead of the new episode's (the one-wavefront kernel's re-spawn and the reset kernel are right).  The site is the auto-reset
  branch block_policy_step keeps for itself (profiles/episode_start_refactor.md says why); the reset and the SameStep re-spawn
  kernel run block_begin_episode and stay right.
* `wide_respawn_sum_stops_short` -- the wide kernel's re-spawn (wide_begin_episode: the step's branch and the SameStep kernel) sums
  the steps of the vehicles BEFORE vehicle vi only (`k < vi[h]`): every x lacks its own step (the reset kernel and the workgroup
  kernel's re-spawn are right).  Named row: N = 192 under `block_kernel` 2, three vehicles per thread -- the `block_kernel` 0 and 1
  rows of that size run the workgroup kernel and pass on this mutant.
* `wide_respawn_speed_in_the_step_row` -- the re-spawn writes info["speed"] to row e instead of row eo of the output planes.  The
  two are the same row in a step launch; only the rollout build (row k * E + e) shows it, in entry point (c).  Named row: N = 256
  under `block_kernel` 2, four vehicles per thread.  The site is the agent rows the straight-road forms share (hwy_device.h:
  begin_agent_rows), so the one-wavefront and the workgroup kernel carry the mutant too; the named row is still the wide
  kernel's.  The re-spawn SOURCE of the rollout builds is the step builds' (one function, called in a loop), so this is the one
  mutant of a re-spawn that only a rollout can see.

What the suite did with these mutants before tests/test_spawn_paths.py existed was established by running the CPU tests of
tests/test_device_reset.py, test_wide_kernel.py, test_rollout.py, test_kernel_variants.py, test_schedule_independence.py,
test_full_size_properties.py and test_families_edge_cases.py (the Linear mutant: test_traffic_parity.py, test_families_edge_cases.py,
test_families_full_size.py, test_rollout.py) against the same mutant libraries once:

* `draw_index_wraps_at_64` SURVIVED all 225 (the one failure, test_workgroup_kernel_abort_chain_against_its_literal_build, compiles
  its second library from the unmutated tree: a real bug would sit in both).
* `workgroup_linear_respawn_draws_episode_0` SURVIVED all 74.
* `wide_respawn_sum_stops_short` was killed by tests/test_wide_kernel.py (wide against workgroup, bit for bit: the two re-spawns no
  longer agree) -- which of the two is right, only the rule says.
* `wide_respawn_speed_in_the_step_row` was killed by tests/test_rollout.py::test_k_steps_on_the_workgroup_kernel (rollout against
  steps, bit for bit)."""
import re

import pytest

from tests import mutation_util

ROW_WIDE = "idm-n65-l6-a2-bk0-fast"          # IDM, N = 65: the wide kernel with K = 2 vehicles per thread
ROW_WIDE_K3 = "idm-n192-l6-a1-bk2"           # IDM, N = 192, block_kernel 2: the wide kernel with K = 3 (hwy_step / rollout_wide_kernel<3, 1>)
ROW_WIDE_K4 = "idm-n256-l6-a1-bk2-fast"      # IDM, N = 256, block_kernel 2: the wide kernel with K = 4 (<4, 1>)
ROW_LINEAR_WORKGROUP = "Aggressive-n65-l6-a1-fast"   # Linear traffic, N = 65: the workgroup kernel with two wavefronts
MUTANTS = {
    "draw_index_wraps_at_64": ("emu_engine.cpp", "HWY_EMU_LIB", ROW_WIDE, [
        ("hwy_device.h", "philox_uniform2(seed, (uint32_t)vi, episode, 0u, &u_lane, &u_speed);",
         "philox_uniform2(seed, (uint32_t)(vi & 63), episode, 0u, &u_lane, &u_speed);")]),
    "workgroup_linear_respawn_draws_episode_0": ("emu_traffic.cpp", "HWY_EMU_TRAFFIC_LIB", ROW_LINEAR_WORKGROUP, [
        ("hwy_device.h", "if (active) spawn_behavior(p, la, e, i, p.rp.base_seed + (uint64_t)e, episode, (me.flags & HWY_F_CONTROLLED) != 0);",
         "if (active) spawn_behavior(p, la, e, i, p.rp.base_seed + (uint64_t)e, 0u, (me.flags & HWY_F_CONTROLLED) != 0);")]),
    "wide_respawn_sum_stops_short": ("emu_engine.cpp", "HWY_EMU_LIB", ROW_WIDE_K3, [
        ("hwy_wave2.h", "for (int k = 0; k <= vi[h] && k < N; ++k) x += sh.x[k];", "for (int k = 0; k < vi[h] && k < N; ++k) x += sh.x[k];")]),
    "wide_respawn_speed_in_the_step_row": ("emu_engine.cpp", "HWY_EMU_LIB", ROW_WIDE_K4, [
        ("hwy_device.h", "if (p.info_speed) p.info_speed[(size_t)eo * p.A + a] = o.v;",
         "if (p.info_speed) p.info_speed[(size_t)e * p.A + a] = o.v;")]),
}
# what each mutant's row must say when it dies (a regular expression: the plane that differs, or the entry point)
DIES_WITH = {"draw_index_wraps_at_64": r"^E\s+lane$", "workgroup_linear_respawn_draws_episode_0": "behaviour parameters",
             "wide_respawn_sum_stops_short": r"^E\s+x$", "wide_respawn_speed_in_the_step_row": "rollout step \\d: info speed"}


def selection(row):
    return [f"tests/test_spawn_paths.py::test_every_spawn_path_follows_the_reference_rule[{row}-emu]"]


def build_mutant(name: str) -> str:
    driver, _, _, sites = MUTANTS[name]
    return mutation_util.build_mutant(sites, driver, f"libhwy_emu_spawn_mut_{name}.so")


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_the_spawn_paths_kill_the_mutant(mutant):
    from concurrent.futures import ThreadPoolExecutor
    from tests.emu import emu
    emu.build_all()  # (the suite's own emulator builds, before two processes could both start one)
    _, env_var, row, _ = MUTANTS[mutant]
    with ThreadPoolExecutor(2) as pool:   # the control and the mutant side by side (two subprocesses)
        f_good = pool.submit(mutation_util.run_selection, None, selection(row), env_var)
        f_bad = pool.submit(lambda: mutation_util.run_selection(build_mutant(mutant), selection(row), env_var))
        good, bad = f_good.result(), f_bad.result()
    assert good.returncode == 0 and "1 passed" in good.stdout, f"{row} must pass on the unmutated kernel source:\n{good.stdout[-3000:]}"
    assert bad.returncode == 1 and "AssertionError" in bad.stdout and re.search(DIES_WITH[mutant], bad.stdout, re.M), \
        f"mutant {mutant} SURVIVED {row} (rc {bad.returncode}):\n{bad.stdout[-3000:]}"
