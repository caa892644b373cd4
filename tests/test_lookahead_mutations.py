"""Load-bearing checks of the fork and scoring kernels, by the method of tests/test_ttc_mutations.py: a rule is broken in a COPY of
the kernel source (one text replacement in hwy_lookahead.h), the CPU emulator (tests/emu/emu_lookahead.cpp) is built from the copy,
and the named tests must FAIL on it -- while they pass on the unmutated source:

* `fork_skips_timer`  -- the fifth f64 plane (the IDM lane-change timer) is not copied;
* `fork_skips_time`   -- the environment's clock is not copied (la_trunc: the branches would never be truncated);
* `no_mask`           -- rewards after the end of an episode keep counting;
* `mask_one_early`    -- the terminal step's reward is dropped;
* `tie_takes_last`    -- among equal maxima the highest branch / first action wins;
* `fused_return`      -- g + d * r in one expression: one rounding where numpy has two.

Each case runs the real test functions in a subprocess with HWY_EMU_LOOKAHEAD_LIB pointing at the mutant."""
import pytest

from tests import mutation_util

H = "hwy_lookahead.h"
MUTANTS = {
    "fork_skips_timer": [(H, "  for (int f = 0; f < p.n_f64; ++f) {\n", "  for (int f = 0; f < p.n_f64; ++f) {\n    if (f == 4) continue;\n")],
    "fork_skips_time": [(H, "    p.dst_time[j] = p.src_time[s];\n", "")],
    "no_mask": [(H, "    if (alive) {\n      const double t = d * p.reward[at * p.A + a];", "    {\n      const double t = d * p.reward[at * p.A + a];")],
    "mask_one_early": [(H, "    if (alive) {\n      const double t = d * p.reward[at * p.A + a];",
                        "    if (alive && !(p.terminated[at] | p.truncated[at])) {\n      const double t = d * p.reward[at * p.A + a];")],
    "tie_takes_last": [(H, "sh_arg[lane] = 0x7fffffff;", "sh_arg[lane] = -1;"),
                       (H, "__hip_atomic_fetch_min(&sh_arg[0], b,", "__hip_atomic_fetch_max(&sh_arg[0], b,"),
                       (H, "__hip_atomic_fetch_min(&sh_arg[1], i,", "__hip_atomic_fetch_max(&sh_arg[1], i,")],
    "fused_return": [(H, "      const double t = d * p.reward[at * p.A + a];\n      g = g + t;", "      g = fma(d, p.reward[at * p.A + a], g);")],
}
FORK = ["tests/test_lookahead_fork.py", "-m", "not gpu"]
PARITY = ["tests/test_lookahead_parity.py", "-m", "not gpu"]
SCORE = ["tests/test_lookahead_score.py", "-m", "not gpu"]
CASES = [
    ("fork_skips_timer", FORK + ["-k", "test_fork_is_the_host_route and n21"]),
    ("fork_skips_time", PARITY + ["-k", "test_per_step_rewards_and_flags and la_trunc"]),
    ("fork_skips_time", FORK + ["-k", "test_fork_is_the_host_route and n8"]),
    ("no_mask", PARITY + ["-k", "test_returns_and_best_action and la_fast"]),
    ("no_mask", SCORE + ["-k", "test_an_episode_that_ends_is_absorbing"]),
    ("mask_one_early", PARITY + ["-k", "test_returns_and_best_action and la_v0"]),
    ("mask_one_early", SCORE + ["-k", "test_an_episode_that_ends_is_absorbing"]),
    ("tie_takes_last", SCORE + ["-k", "test_scores_equal_the_restatement_bit_for_bit and B25"]),
    ("tie_takes_last", PARITY + ["-k", "test_returns_and_best_action and la_fast"]),
    ("fused_return", SCORE + ["-k", "test_fused_and_unfused_returns_differ_here"]),
]


def build_mutant(name: str) -> str:
    return mutation_util.build_mutant(MUTANTS[name], "emu_lookahead.cpp", f"libhwy_emu_lookahead_mut_{name}.so")


def run_selection(lib, selection):
    return mutation_util.run_selection(lib, selection, "HWY_EMU_LOOKAHEAD_LIB")


def _build_the_suites_own():
    from tests.emu import emu
    emu.build_all()  # (before two processes could both start one)


@pytest.mark.parametrize("mutant,selection", CASES, ids=[f"{c[0]}-{c[1][0].split('_')[-1][:-3]}" for c in CASES])
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
