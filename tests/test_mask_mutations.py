"""Load-bearing checks of the action-mask kernel, by the method of tests/test_ttc_mutations.py: a rule of the reference's
``get_available_actions`` / ``is_reachable_from`` is broken in a COPY of the kernel source (one text replacement in hwy_mask.h), the
CPU emulator (tests/emu/emu_mask.cpp) is built from the copy, and the comparison with the fixture that covers the rule must FAIL on
it -- while it passes on the unmutated source (tests/test_mask_parity.py):

* `top_speed_inclusive`  -- FASTER stays available AT the top speed index (`<=` for `<`): mask_placed, mask_speeds2;
* `left_right_swapped`   -- the two lane columns change places: mask_placed, mask_lanes2;
* `forbidden_ignored`    -- a forbidden lane counts as reachable: mask_merge, next to the ramp lane ("b", "c", 2);
* `no_length_margin`     -- `s < length` instead of `s < length + VEHICLE_LENGTH`: test_length_margin below, a hand-placed ego within
  the last 5 m behind the end of ("a", "b") of merge-v0, where the side lane is still in reach;
* `target_lane_used`     -- the rule reads the vehicle's target lane instead of its current lane: mask_fast, during a lane change.
The emulator is loaded in-process next to the suite's own."""
import numpy as np
import pytest

from tests import mask_util, mutation_util
from tests.emu import emu
from tests.mask_util import MaskGolden

H = "hwy_mask.h"
MUTANTS = {
    "top_speed_inclusive": [(H, "faster = longitudinal && sidx < p.n_ts - 1;", "faster = longitudinal && sidx <= p.n_ts - 1;")],
    "left_right_swapped": [(H, "out[0] = left ? 1 : 0; out[1] = 1; out[2] = right ? 1 : 0;", "out[0] = right ? 1 : 0; out[1] = 1; out[2] = left ? 1 : 0;")],
    "forbidden_ignored": [(H, "if (l.forbidden) return false;", "if (false && l.forbidden) return false;")],
    "no_length_margin": [(H, "0 <= s && s < l.length + HWY_VEH_LENGTH;", "0 <= s && s < l.length;")],
    "target_lane_used": [(H, "const int lane = ix ? ix_word_lane(w) : word_lane(w),", "const int lane = ix ? ix_word_lane(w) : word_target(w),")],
}
CASES = [("top_speed_inclusive", "mask_placed"), ("top_speed_inclusive", "mask_speeds2"), ("left_right_swapped", "mask_placed"),
         ("left_right_swapped", "mask_lanes2"), ("forbidden_ignored", "mask_merge"), ("target_lane_used", "mask_fast")]
_libs = {}


def mutant(name: str):
    if name not in _libs:
        _libs[name] = emu.load("mask", mutation_util.build_mutant(MUTANTS[name], "emu_mask.cpp", f"libhwy_emu_mask_mut_{name}.so"))
    return _libs[name]


def mismatches(g: MaskGolden, L=None) -> int:
    cfg = g.hwy_config()
    return sum(int((emu.action_mask(cfg, g.state(i), L) != g.mask(i)).sum()) for i in g.indices())


@pytest.mark.parametrize("name,fixture", CASES, ids=[f"{m}-{f}" for m, f in CASES])
def test_broken_rule_fails_the_fixture_that_covers_it(name, fixture):
    g = MaskGolden(fixture)
    assert mismatches(g) == 0, "the comparison must pass on the unmutated kernel source"
    assert mismatches(g, mutant(name)) > 0, f"mutant {name} SURVIVED {fixture}"


def end_of_lane_state(g: MaskGolden, s_past_end: float) -> dict:
    """The reset state of mask_merge with the ego of environment 0 on ("a", "b", 1), `s_past_end` metres past the lane's end."""
    from highwayenv_amd import merge
    tab = merge.table_from_config(g.hwy_config())
    st = g.state(None)
    st["x"][0, 0] = tab["x0"][1] + tab["length"][1] + s_past_end
    st["lane"][0, 0] = st["target_lane"][0, 0] = 1
    return st


def test_length_margin():
    """Within VEHICLE_LENGTH behind the end of its lane the ego can still change to the side lane (lane.py:116: s < length +
    LENGTH); past that margin it cannot.  The reference's own rule, evaluated here on the lane table; the mutant loses the margin."""
    g = MaskGolden("mask_merge")
    cfg = g.hwy_config()
    inside, outside = end_of_lane_state(g, 3.0), end_of_lane_state(g, 5.5)
    assert emu.action_mask(cfg, inside)[0, 0, 0] and not emu.action_mask(cfg, outside)[0, 0, 0]
    assert not emu.action_mask(cfg, inside, mutant("no_length_margin"))[0, 0, 0]


# ---- the masked optimistic planner (csrc/hwy_opd.h: opd_tree_step<CAP, true>) -------------------------------------------------------
# * `masked_child_ingested`  -- a child whose action is unavailable is created and ingested anyway (the unmasked search under the flag);
# * `argmax_reads_uncreated` -- the maximum the plan follows from a node down is taken over all n slots, never-created ones included.
# Each must fail the comparison with the plain Python restatement (tests/test_opd_mask.py: the masked search equals it bit for bit).
O = "hwy_opd.h"
OPD_MUTANTS = {
    "masked_child_ingested": [(O, "p.child_mask[(size_t)e * n * n + (i - 1) % n] : p.created[row + i]) != 0;",
                               "p.child_mask[(size_t)e * n * n + (i - 1) % n] : p.created[row + i]) != 0 || true;"),
                              (O, "if (!available) continue;  // no child: nothing is ingested", "(void)available;")],
    "argmax_reads_uncreated": [(O, "if (sh_exp[1 + j * n + a] != -2) __hip_atomic_fetch_max(&sh_key[0], score_key(sh_lo[1 + j * n + a]),",
                                "if (true) __hip_atomic_fetch_max(&sh_key[0], score_key(sh_lo[1 + j * n + a]),")],
}


@pytest.mark.parametrize("name", sorted(OPD_MUTANTS))
def test_broken_masked_search_fails_the_restatement(name):
    from tests import opd_mask_util as omu
    from tests.emu import emu
    from tests.test_opd_mask import _env
    env = _env("emu", "lanes3_speeds3")
    want = omu.restate_masked_opd("emu", env, 50, 0.7)
    assert want["masked_out"].sum() > 0
    action, got = env.plan_opd(50, 0.7, return_details=True, masked=True)
    omu.assert_plan_equals(action, got, want, "the unmutated kernel source")
    env._engine.opd_lib = emu.load("opd", mutation_util.build_mutant(OPD_MUTANTS[name], "emu_opd.cpp", f"libhwy_emu_opd_mask_mut_{name}.so"))
    action, got = env.plan_opd(50, 0.7, return_details=True, masked=True)
    with pytest.raises(AssertionError):
        omu.assert_plan_equals(action, got, want, name)
    env.close()
