"""Load-bearing checks of the act kernel (csrc/hwy_act.h), by the method of tests/test_control_mutations.py: a rule is broken in a
COPY of the kernel source (one text replacement), the CPU emulation (tests/emu/emu_continuous.cpp) is built from the copy, and a
selection of the continuous tests runs against it in a subprocess -- it must FAIL, while it passes on the intact source:

* `in_double`   -- the mapping done in double instead of float32, operation by operation: caught by the reference fixture whose
  range ends are not float32 numbers (tests/test_continuous_parity.py, cont_asym) -- the stored pair after the act launch;
* `no_clip`     -- np.clip dropped: caught by the fixtures' actions beyond [-1, 1] (cont_fast, free running);
* `wrong_slot`  -- every agent's steering written to agent 0's slot of its environment: caught by the two-agent rows of the
  comparison with the NumPy restatement (tests/test_continuous_act.py)."""
import pytest

from tests import mutation_util

MUTANTS = {
    "in_double": [("hwy_act.h", "  const float o = (float)y0 + t;\n  return (double)o;\n",
                   "  (void)t;\n  return y0 + ((double)x + 1.0) * (y1 - y0) / 2.0;\n")],
    "no_clip": [("hwy_act.h", "const float x = fminf(fmaxf(v, -1.0f), 1.0f);", "const float x = v;")],
    "wrong_slot": [("hwy_act.h", "p.ctl_steer[r] = steer;", "p.ctl_steer[r - r % p.A] = steer;")],
}
SELECTIONS = {
    "in_double": ["tests/test_continuous_parity.py", "-k", "teacher_forced and cont_asym and emu"],
    "no_clip": ["tests/test_continuous_parity.py", "-k", "free_running and cont_fast and emu"],
    "wrong_slot": ["tests/test_continuous_act.py", "-k", "bit_for_bit and emu and 2-axes"],
}
ENV = "HWY_EMU_CONTINUOUS_LIB"


def test_intact_source_passes_every_selection():
    for name, selection in SELECTIONS.items():
        r = mutation_util.run_selection(None, selection, ENV)
        assert r.returncode == 0 and " passed" in r.stdout, f"{name}: {r.stdout[-2000:]}{r.stderr[-2000:]}"


@pytest.mark.parametrize("name", list(MUTANTS))
def test_seeded_bug_fails_its_selection(name):
    lib = mutation_util.build_mutant(MUTANTS[name], "emu_continuous.cpp", f"libhwy_emu_continuous_mut_{name}.so")
    r = mutation_util.run_selection(lib, SELECTIONS[name], ENV)
    assert r.returncode == 1 and " failed" in r.stdout, f"the mutant {name} survived: {r.stdout[-2000:]}{r.stderr[-2000:]}"
    assert "AssertionError" in r.stdout or "Mismatch" in r.stdout or "not equal" in r.stdout, r.stdout[-2000:]
