"""Load-bearing checks of the optimistic planner's kernel, by the method of tests/test_ttc_mutations.py: a rule is broken in a COPY
of the kernel source (text replacements in hwy_opd.h), the CPU emulator (tests/emu/emu_opd.cpp) is built from the copy, and the
named cases of tests/test_opd_parity.py must FAIL on it -- while they pass on the unmutated source:

* `tie_takes_highest`  -- among equal maxima the highest node index / action id wins;
* `done_leaf_expanded` -- a selected leaf that is done is expanded like any other;
* `backup_last_child`  -- an expanded node takes the bounds of its last child instead of the maximum over its children;
* `disc_not_advanced`  -- a child keeps its parent's discount.

Each case runs the real test functions in a subprocess with HWY_EMU_OPD_LIB pointing at the mutant."""
import pytest

from tests import mutation_util

H = "hwy_opd.h"
MUTANTS = {
    "tie_takes_highest": [(H, "  if (lane == 0) sh_arg = 0x7fffffff;\n  __syncthreads();", "  if (lane == 0) sh_arg = -1;\n  __syncthreads();"),
                          (H, "      if (lane == 0) sh_arg = 0x7fffffff;\n", "      if (lane == 0) sh_arg = -1;\n"),
                          (H, "__hip_atomic_fetch_min(&sh_arg, i,", "__hip_atomic_fetch_max(&sh_arg, i,"),
                          (H, "__hip_atomic_fetch_min(&sh_arg, a,", "__hip_atomic_fetch_max(&sh_arg, a,")],
    "done_leaf_expanded": [(H, "const bool is_void = sh_done[leaf] != 0;", "const bool is_void = false;")],
    "backup_last_child": [(H, "sh_lo[node] = score_unkey(sh_key[0]);", "sh_lo[node] = sh_lo[j * n + n];"),
                          (H, "sh_up[node] = score_unkey(sh_key[1]);", "sh_up[node] = sh_up[j * n + n];")],
    "disc_not_advanced": [(H, "const double disc = disc_p * p.gamma;", "const double disc = disc_p;")],
}
PARITY = ["tests/test_opd_parity.py", "-m", "not gpu"]
CASES = [
    ("tie_takes_highest", PARITY + ["-k", "test_terminal_leaves_solved_trees_and_ties and lane0"]),
    ("tie_takes_highest", PARITY + ["-k", "test_plan_equals_the_restated_rules and b85"]),
    ("done_leaf_expanded", PARITY + ["-k", "test_terminal_leaves_solved_trees_and_ties and short"]),
    ("backup_last_child", PARITY + ["-k", "test_plan_equals_the_restated_rules and b15_three"]),
    ("disc_not_advanced", PARITY + ["-k", "test_plan_equals_the_restated_rules and b15_three"]),
    ("disc_not_advanced", PARITY + ["-k", "test_plan_equals_the_restated_rules and b5_one"]),
]


def build_mutant(name: str) -> str:
    return mutation_util.build_mutant(MUTANTS[name], "emu_opd.cpp", f"libhwy_emu_opd_mut_{name}.so")


def run_selection(lib, selection):
    return mutation_util.run_selection(lib, selection, "HWY_EMU_OPD_LIB")


def _build_the_suites_own():
    from tests.emu import emu
    emu.build_all()  # (before two processes could both start one)


@pytest.mark.parametrize("mutant,selection", CASES, ids=[f"{c[0]}-{c[1][-1].split(' and ')[-1]}" for c in CASES])
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
