"""Mutation check of the parity rules (round-3 verdict): the randomised engine-vs-oracle comparisons tolerate -- and count -- a
few knife-edge cases of the reference itself (a push direction, a touching pair, a lane index or a queue order decided by the
last bit).  Could those rules hide a real defect?  Four bugs are seeded into the kernel SOURCE, the CPU emulator is built from
each mutated copy (tests/emu: the same headers the GPU build compiles), and the comparison that covers the mutated path must
FAIL on it -- while passing on the unmutated build:

* `ix_first_pair_wins`   -- the intersection kernel keeps the impact of the LOWEST partner slot (the reference's loop
  overwrites: the last pair wins, objects.py:104-112): only visible in pile-ups, where the exemption rules live;
* `net_pair_list_carry`  -- the road-network kernel's pair list carries the overflow of a pass (> 64 close pairs) to the next
  pass shifted by one entry: only visible with more close pairs than one pass holds;
* `mobil_sides_swapped`  -- the one-wavefront kernel weighs the LEFT lane change with the right lane's gap and vice versa
  (behavior.py:265-324);
* `reach_ignores_motion` -- the forward collision walk of the three highway kernels stops at the pre-check radius of bodies at rest,
  forgetting what the frame moved them (road.py:477-481 tests ALL pairs): only visible with bodies that close a gap within one frame;
* `chain_compares_in_lds` -- an ORDERING bug: the workgroup kernel's abort-chain loop tests for its fixed point against the
  previous round's verdicts where they lie in LDS -- the half of the slot pair a wavefront that runs ahead already rewrites with
  the next round's.  The emulator's default round-robin schedule never lets a wavefront run ahead, so the suite's depth-two
  chain test passes on it; the wave orders of tests/test_schedule_independence.py must catch it.

Each case runs the real test functions in a subprocess with HWY_EMU_LIB pointing at the mutant."""
import pytest

from tests import mutation_util

MUTANTS = {
    "ix_first_pair_wins": [
        ("hwy_ix.h", "__hip_atomic_fetch_max(&sh.jmax[a], b, __ATOMIC_RELAXED", "__hip_atomic_fetch_min(&sh.jmax[a], b, __ATOMIC_RELAXED"),
        ("hwy_ix.h", "__hip_atomic_fetch_max(&sh.jmax[b], a, __ATOMIC_RELAXED", "__hip_atomic_fetch_min(&sh.jmax[b], a, __ATOMIC_RELAXED"),
        ("hwy_ix.h", "if (i < SH::kCap) { sh.jmax[i] = -1; sh.flag[i] = 0; }", "if (i < SH::kCap) { sh.jmax[i] = 0x7fffffff; sh.flag[i] = 0; }"),
        ("hwy_ix.h", "const int j_imp = i < SH::kCap ? sh.jmax[i] : -1;",
         "const int j_imp = (i < SH::kCap && sh.jmax[i] != 0x7fffffff) ? sh.jmax[i] : -1;")],
    "net_pair_list_carry": [
        ("hwy_net.h", "const int carry = i < left ? (int)plist[count + i] : 0,", "const int carry = i < left ? (int)plist[count + i + 1] : 0,")],
    "reach_ignores_motion": [   # (round 6: the forward collision walk's reach from the frame's maxima, hwy_device.h reach_from_keys)
        ("hwy_device.h", "return ((5.5 + S * dt) + 2.0 * D) + 1e-6;", "return ((5.5 + 0.0 * S * dt) + 0.0 * D) + 1e-6;")],
    "chain_compares_in_lds": [   # (hwy_device.h section D: the fixed-point test against the LDS half the next round rewrites)
        ("hwy_device.h", "same = same && v == last[w];", "same = same && v == (prev ? prev[w] : (u64)0);")],
    "mobil_sides_swapped": [   # (the compacted MOBIL tasks of round 6: side 0 = left reads row lane, side 1 = right row lane + 2)
        ("hwy_wave.h", "const u64 m = sh.lane_mask[ln + (side ? 2 : 0)];", "const u64 m = sh.lane_mask[ln + (side ? 0 : 2)];")],
}
# (mutant, pytest selection, extra environment, must the selection pass?)  The selections are the suite's own tests: the fuzz families
# at their default chunk numbers (what `pytest -m gpu` runs on the GPU box, here on the emulator) and the directed pile-up test.
FUZZ = {"HWY_FUZZ_BACKEND": "emu", "HWY_FUZZ_FIRST": "0", "HWY_FUZZ_CHUNKS": "1"}
CASES = [
    # (chunk 0 holds no frame in which one vehicle is hit by two others; chunk 1 does -- one chunk is 30 s on the emulator)
    ("ix_first_pair_wins", ["tests/test_fuzz_configs.py", "-m", "gpu", "-k", "intersection"], dict(FUZZ, HWY_FUZZ_FIRST="1")),
    ("net_pair_list_carry", ["tests/test_pileup.py", "-m", "not gpu", "-k", "merge"], {}),
    ("mobil_sides_swapped", ["tests/test_fuzz_configs.py", "-m", "gpu", "-k", "test_random_configurations_vs_oracle"], FUZZ),
    ("reach_ignores_motion", ["tests/test_collision_steps.py", "-m", "not gpu", "-k", "fast_bodies_are_not_missed"], {}),
    ("chain_compares_in_lds", ["tests/test_schedule_independence.py", "-m", "not gpu", "-k", "abort_chain_vs_oracle and n90_spread"], {}),
]
# the ordering bug survives what the default schedule runs: the depth-two chain on every kernel family against the oracle
ROUND_ROBIN_SURVIVORS = [
    ("chain_compares_in_lds", ["tests/test_wide_kernel.py", "-m", "not gpu", "-k", "abort_chain_of_depth_two_vs_oracle"]),
]


def build_mutant(name: str) -> str:
    return mutation_util.build_mutant(MUTANTS[name], "emu_engine.cpp", f"libhwy_emu_mut_{name}.so")


def run_selection(lib, selection, env_extra):
    return mutation_util.run_selection(lib, selection, "HWY_EMU_LIB", env_extra)


@pytest.mark.parametrize("mutant,selection,env_extra", CASES, ids=[c[0] for c in CASES])
def test_seeded_bug_fails_the_comparison_that_covers_it(mutant, selection, env_extra):
    from concurrent.futures import ThreadPoolExecutor
    from tests.emu import emu
    emu.build()   # (the suite's own emulator build, before two processes could both start building it)
    with ThreadPoolExecutor(2) as pool:   # the control and the mutant side by side (two subprocesses)
        f_good = pool.submit(run_selection, None, selection, env_extra)
        f_bad = pool.submit(lambda: run_selection(build_mutant(mutant), selection, env_extra))
        good, bad = f_good.result(), f_bad.result()
    assert good.returncode == 0, f"the selection must pass on the unmutated kernel source:\n{good.stdout[-3000:]}"
    assert bad.returncode == 1 and "AssertionError" in bad.stdout, \
        f"mutant {mutant} SURVIVED {selection} (rc {bad.returncode}):\n{bad.stdout[-3000:]}"


@pytest.mark.parametrize("mutant,selection", ROUND_ROBIN_SURVIVORS, ids=[c[0] for c in ROUND_ROBIN_SURVIVORS])
def test_ordering_bug_survives_the_round_robin_schedule(mutant, selection):
    """The other half of the ordering case above: on the default schedule the mutant PASSES a comparison that covers the mutated
    code -- only the schedules that let one wavefront run ahead tell it apart."""
    from tests.emu import emu
    emu.build()
    res = run_selection(build_mutant(mutant), selection, {})
    assert res.returncode == 0 and " passed" in res.stdout, \
        f"mutant {mutant} was expected to pass {selection} on the round-robin schedule (rc {res.returncode}):\n{res.stdout[-3000:]}"
