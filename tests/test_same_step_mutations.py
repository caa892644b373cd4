"""Load-bearing checks of the SameStep sequence and its re-spawn kernels, by the method of tests/test_mask_mutations.py: a rule is
broken in a COPY of the kernel source (one text replacement), the CPU emulation (tests/emu/emu_same_step.cpp) is built from the copy,
and the comparison of one same-step call against two next-step calls (tests/same_step_util.py: one_call_against_two) must FAIL on
it -- while it passes on the unmutated source (tests/test_same_step_device.py):

* `same_episode`   -- the re-spawn draws from the stream of `episode` instead of `episode + 1` (and stores that number).  The number
  is formed once for every kernel form (hwy_device.h: episode_stream), so the four mutants are one site and one library; each
  row runs it through another form's *_begin_episode: the one-wavefront kernel (`fast`), the wide kernel (`n65`), the workgroup
  kernel (`n129`) and the road-network kernel (`merge`);
* `stash_late`     -- the stash runs after the re-spawn instead of before it: the terminal rows are gone, the mark is cleared;
* `clears_reward`  -- the re-spawn zeroes the reward of the row, as the next-step mode does.  The straight-road forms share their
  agent rows (hwy_device.h: begin_agent_rows), so one mutant covers the three of them (run on `fast`); the road network writes its
  own (`i < A`) and has its own mutant, `clears_reward_net` (`merge`).
The mutated functions are shared with the next-step branch of the step kernels and with the reset kernels, but only engine Y runs
the mutant; X, the yardstick, is the unmutated next-step emulation."""
import pytest

from tests import mutation_util, same_step_util as ssu
from tests.emu import emu

NEXT = "s.episode = M == Begin::Reset ? 0u : p.st.episode[e] + 1u;  // the next episode's stream"
SAME = "s.episode = M == Begin::Reset ? 0u : p.st.episode[e];  // the next episode's stream"
SAME_EPISODE = [("hwy_device.h", NEXT, SAME)]
MUTANTS = {
    "same_episode_wave": SAME_EPISODE,
    "same_episode_wide": SAME_EPISODE,
    "same_episode_block": SAME_EPISODE,
    "same_episode_net": SAME_EPISODE,
    "stash_late": [("hwy_same_step.h", "  if (int rc = ops.stash()) return rc;\n  if (int rc = ops.respawn()) return rc;\n",
                    "  if (int rc = ops.respawn()) return rc;\n  if (int rc = ops.stash()) return rc;\n")],
    "clears_reward": [("hwy_device.h", "if (M == Begin::NextStep) p.reward[(size_t)eo * p.A + a] = 0.0;",
                       "if (M != Begin::Reset) p.reward[(size_t)eo * p.A + a] = 0.0;")],
    "clears_reward_net": [("hwy_net.h", "if (M == Begin::NextStep) p.reward[(size_t)eo * p.A + i] = 0.0;",
                           "if (M != Begin::Reset) p.reward[(size_t)eo * p.A + i] = 0.0;")],
}
CASES = [("same_episode_wave", "fast"), ("same_episode_wide", "n65"), ("same_episode_block", "n129"), ("same_episode_net", "merge"),
         ("stash_late", "fast"), ("clears_reward", "fast"), ("clears_reward_net", "merge")]
_libs = {}


def mutant(name: str):
    key = str(MUTANTS[name])  # (mutants of one site share a library)
    if key not in _libs:
        import tests.emu.emu_same_step  # noqa: F401  (registers the unit)
        _libs[key] = emu.load("same_step", mutation_util.build_mutant(MUTANTS[name], "emu_same_step.cpp", f"libhwy_emu_same_step_mut_{name}.so"))
    return _libs[key]


def _mutated_engine(name):
    def make(cfg):
        eng = ssu.make_engine("emu", cfg)
        eng.same_step_lib = mutant(name)
        return eng
    return make


@pytest.mark.parametrize("name,config", CASES, ids=[f"{m}-{c}" for m, c in CASES])
def test_seeded_bug_fails_the_one_call_comparison(name, config):
    seed, warmup, action, stagger = ssu.ENTRIES[config][0]
    ssu.one_call_against_two("emu", config, seed, warmup, action, stagger)  # must pass on the unmutated source
    with pytest.raises(AssertionError):  # ("DID NOT RAISE": the mutant survived)
        ssu.one_call_against_two("emu", config, seed, warmup, action, stagger, make_y=_mutated_engine(name))
