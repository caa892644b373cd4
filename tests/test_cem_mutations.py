"""Load-bearing checks of the CEM kernels (csrc/hwy_cem.h), by the method of tests/test_continuous_mutations.py: a rule is broken in
a COPY of the kernel source (one text replacement), the CPU emulation (tests/emu/emu_cem.cpp) is built from the copy, and a
selection of the CEM tests runs against it in a subprocess -- it must FAIL, while it passes on the intact source:

* `ties_high`     -- ties between equal returns broken toward the HIGHEST branch: caught where every return ties while the
  samples differ (tests/test_cem_plan.py: test_equal_returns_break_toward_the_lowest_branch -- the refit and the best sequence);
* `bessel`        -- the variance divided by M - 1: caught by the restatement's std (test_plan_equals_the_restatement_bit_for_bit);
* `same_noise`    -- the Philox counter ignoring the iteration: caught by the noise of iterations 1 and 2 against the NumPy
  Box-Muller on the Python Philox (the same test, a case with three iterations)."""
import pytest

from tests import mutation_util

MUTANTS = {
    "ties_high": [("hwy_cem.h", "(other == mine && o < b)", "(other == mine && o > b)")],
    "bessel": [("hwy_cem.h", "const double v = acc / count;", "const double v = acc / (count - 1.0);")],
    "same_noise": [("hwy_cem.h", "(uint32_t)(p.iter * HWY_CEM_MAX_HORIZON + k)", "(uint32_t)k")],
}
SELECTIONS = {
    "ties_high": ["tests/test_cem_plan.py", "-k", "test_equal_returns_break_toward_the_lowest_branch and emu"],
    "bessel": ["tests/test_cem_plan.py", "-k", "test_plan_equals_the_restatement_bit_for_bit and emu and B5-M2-K3-s2-I3"],
    "same_noise": ["tests/test_cem_plan.py", "-k", "test_plan_equals_the_restatement_bit_for_bit and emu and B5-M2-K3-s2-I3"],
}
ENV = "HWY_EMU_CEM_LIB"


def test_intact_source_passes_every_selection():
    for name, selection in SELECTIONS.items():
        r = mutation_util.run_selection(None, selection, ENV)
        assert r.returncode == 0 and " passed" in r.stdout, f"{name}: {r.stdout[-2000:]}{r.stderr[-2000:]}"


@pytest.mark.parametrize("name", list(MUTANTS))
def test_seeded_bug_fails_its_selection(name):
    lib = mutation_util.build_mutant(MUTANTS[name], "emu_cem.cpp", f"libhwy_emu_cem_mut_{name}.so")
    r = mutation_util.run_selection(lib, SELECTIONS[name], ENV)
    assert r.returncode == 1 and " failed" in r.stdout, f"the mutant {name} survived: {r.stdout[-2000:]}{r.stderr[-2000:]}"
    assert "AssertionError" in r.stdout or "Mismatch" in r.stdout or "not equal" in r.stdout, r.stdout[-2000:]
