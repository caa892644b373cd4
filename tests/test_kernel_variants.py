"""Every register-allocation build of the step and rollout kernels is executed, and computes what the engine's default build computes.

The step, rollout and workgroup kernels are compiled once per WPE (``__launch_bounds__(threads, WPE)``); ``hwy_create`` picks the
build from the batch size or from ``hwy_config.tune_waves_per_eu``.  The parity suite runs at small batches, i.e. on ONE build per
kernel (WPE 3 on the straight road, 4 on the road network, 2 on the intersection) -- a different register allocation is where an
uninitialised value, an LDS ordering that holds at one occupancy only, or a wrong spill would change a result.  Here:

1. (CPU) the table of tests/variants_util.py is COMPLETE against the code object's own metadata: every kernel it names exists, and
   every step / rollout kernel of the code object -- the step kernels compiled for the registered configurations (hwy_shape_wave_kernel)
   among them -- is named by some (row, value) or listed below with the reason it has one build;
2. every (row, value) runs on the MI355X, step() and rollout(), with auto-reset inside the run, and is EQUAL -- outputs of every
   step, final state, drawn behaviour parameters, stored controls -- to the untuned engine, whose builds the rest of the suite holds
   to the oracle; after every launch the library's own report of the kernel it ran (hwy_last_step_shape) must be what the table
   says, so a row cannot name one kernel while another runs; builds no test has executed are also compared with the oracle directly, free running, at the suite's tolerances;
3. the build the engine itself takes above its batch-size threshold equals the 3- and the 4-wave build;
4. ``tune_extra_lds`` (dynamic LDS on the one-wavefront launches) changes nothing.

The ``emu`` leg (one value against the default: the emulation compiles one build) exercises the plumbing of the knob and this
file's own logic on the CPU."""
import numpy as np
import pytest

from highwayenv_amd import _abi, build, merge
from tests import variants_util as vu
from tests.families_util import rollout

ROWS = vu.rows()


def ident(label: str) -> str:
    return label.replace(" ", "-")


# --------------------------------------------------------------------------- 1. the table against the code object

# Step / rollout kernels that exist in ONE register-allocation build per shape: waves_per_eu does not select among them, so no row
# of the table may claim them.  (Their template argument is that one build's launch bound.)
ONE_BUILD = {
    "hwy::hwy_{}_wide_kernel<2, 2>": "the wide kernel, two vehicles per thread: one build (245 VGPRs, two wavefronts per SIMD)",
    "hwy::hwy_{}_wide_kernel<3, 1>": "the wide kernel, three vehicles per thread: one build, one wavefront per SIMD",
    "hwy::hwy_{}_wide_kernel<4, 1>": "the wide kernel, four vehicles per thread: one build, one wavefront per SIMD",
    "hwy::hwy_net_{}_kernel<3, true>": "road network with the OccupancyGrid observation: one build",
    "hwy::hwy_ix_{}_kernel<2, 64, 64>": "intersection with more than 32 slots: 24 KB of LDS, one build at two wavefronts per SIMD",
}
# Instantiated, but reached by no configuration: none.
UNREACHABLE = {}


@pytest.fixture(scope="module")
def res():
    pytest.importorskip("msgpack")  # (the metadata note is msgpack; present in the build image and on the GPU box)
    if build.is_stale():
        build.build_engine()
    return build.kernel_resources()


def table_kernels() -> dict:
    """{kernel name: [(row label, waves_per_eu), ...]} over the whole table."""
    out = {}
    for label, d, kw in ROWS:
        for v in (1, 2, 3, 4):
            for name in vu.launched(d, vu.with_tuning(kw, waves_per_eu=v), v):
                out.setdefault(name, []).append((label, v))
    return out


def test_every_kernel_the_table_names_is_in_the_code_object(res):
    missing = {k: v for k, v in table_kernels().items() if k not in res}
    assert not missing, missing


def test_every_step_and_rollout_build_is_reached_by_the_table(res):
    """A new family, or a new build of an old one, cannot be added without a row: whatever the code object holds under a step or
    rollout name is launched by some (row, value), has one build (ONE_BUILD) or is listed as unreachable, with a reason."""
    named = table_kernels()
    one_build = {k.format(stage): why for k, why in ONE_BUILD.items() for stage in ("step", "rollout")}
    listed = {**one_build, **UNREACHABLE}
    assert all(why.strip() for why in listed.values())
    in_object = [k for k in res if vu.STEP_OR_ROLLOUT.match(k) or vu.SHAPE_KERNEL.match(k)]
    assert len(in_object) > 100  # (the pattern still finds them)
    # the kernels compiled for the registered configurations: three shapes x four register-allocation builds, every one of them
    # named by a (row, value), and the table names no other; the generic one-wavefront step builds beside them likewise
    shapes = sorted(k for k in in_object if vu.SHAPE_KERNEL.match(k))
    assert shapes == sorted(vu.shape_kernel(s, w) for s in vu.SHAPES for w in (1, 2, 3, 4)), shapes
    assert sorted(k for k in named if vu.SHAPE_KERNEL.match(k)) == shapes
    for w in (1, 2, 3, 4):
        for scan in ("true", "false"):
            assert f"hwy::hwy_step_wave_kernel<{w}, {scan}>" in named and f"hwy::hwy_step_wave_kernel<{w}, {scan}>" in res
    unreached = [k for k in in_object if k not in named and k not in listed]
    assert not unreached, f"step / rollout kernels in the code object that no (row, value) of tests/variants_util.py launches: {unreached}"
    # the exceptions stay honest: each exists, and none is something the table launches after all
    assert not [k for k in listed if k not in res], "listed but not in the code object"
    assert not [k for k in listed if k in named], "listed as an exception, yet launched by the table"
    # and the values the tests loop over reach every build of a row (the intersection's rule maps 1, 2 -> 2 and 3, 4 -> 3)
    for label, d, kw in ROWS:
        all_values = {n for v in (1, 2, 3, 4) for n in vu.launched(d, kw, v)}
        assert {n for v in vu.values(kw) for n in vu.launched(d, kw, v)} == all_values, label


def test_the_restated_selection_on_known_launches():
    """launched() on configurations whose kernel the project's records name (profiles/): the wide kernel, the
    forced workgroup kernel, the one-build kernels."""
    d = _abi.highway_default_config()
    assert vu.launched(dict(d, vehicles_count=100), {}, 3)[0] == "hwy::hwy_step_wide_kernel<2, 2>"
    assert vu.launched(dict(d, vehicles_count=100), dict(vu.BLOCK), 4) == ("hwy::hwy_step_kernel<2, 4>", "hwy::hwy_rollout_kernel<2, 4>")
    assert vu.launched(dict(d, vehicles_count=200), {}, 3)[0] == "hwy::hwy_step_kernel<4, 3>"
    assert vu.launched(dict(d, vehicles_count=200), {"tuning": {"block_kernel": 2}}, 3)[0] == "hwy::hwy_step_wide_kernel<4, 1>"
    assert vu.launched(dict(d, vehicles_count=100, other_vehicles_type=vu.LINEAR), {}, 4)[0] == "hwy::hwy_step_linear_kernel<2, 4>"
    assert vu.launched(dict(d, vehicles_count=50), {"fast": True}, 4)[0] == "hwy::hwy_step_wave_kernel<4, false>"
    assert vu.launched(dict(merge.merge_default_config(), **vu.GRID), {"scenario": "merge"}, 4)[0] == "hwy::hwy_net_step_kernel<3, true>"
    assert vu.launched(vu.ix(40), {"scenario": "intersection"}, 3)[1] == "hwy::hwy_ix_rollout_kernel<2, 64, 64>"
    assert vu.launched(vu.ix(30), {"scenario": "intersection"}, 4)[0] == "hwy::hwy_ix_step_kernel<3, 32, 64>"
    # the registered configurations run the kernel compiled for them (a full step with auto-reset), their rollout the generic one;
    # one field off each -- a fifth lane, 15 frames per step with ego-only collisions, 65 vehicles, the workgroup kernel forced --
    # is the generic kernel again
    fast3, fast4, v0 = _abi.highway_fast_default_config(), dict(_abi.highway_fast_default_config(), lanes_count=4), d
    assert (vu.step_shape(fast3, {"fast": True}), vu.step_shape(fast4, {"fast": True}), vu.step_shape(v0, {})) == (1, 2, 3)
    assert vu.launched(fast3, {"fast": True}, 3) == ("hwy::hwy_shape_wave_kernel<hwy::FixedShape<1, 3, 89, 5>, 3>", "hwy::hwy_rollout_wave_kernel<3, false>")
    assert vu.launched(fast4, {"fast": True}, 1) == ("hwy::hwy_shape_wave_kernel<hwy::FixedShape<2, 4, 89, 5>, 1>", "hwy::hwy_rollout_wave_kernel<1, false>")
    assert vu.launched(v0, {}, 4) == ("hwy::hwy_shape_wave_kernel<hwy::FixedShape<3, 4, 25, 15>, 4>", "hwy::hwy_rollout_wave_kernel<4, true>")
    assert vu.launched(dict(fast3, lanes_count=5), {"fast": True}, 3)[0] == "hwy::hwy_step_wave_kernel<3, false>"
    assert vu.launched(fast3, {}, 3)[0] == "hwy::hwy_step_wave_kernel<3, true>"  # (highway-fast-v0's dict without its collision rule)
    assert vu.launched(dict(fast4, simulation_frequency=15), {"fast": True}, 2)[0] == "hwy::hwy_step_wave_kernel<2, false>"
    assert vu.launched(dict(v0, lanes_count=3), {}, 4)[0] == "hwy::hwy_step_wave_kernel<4, true>"
    assert vu.launched(dict(v0, vehicles_count=64), {}, 3)[0] == "hwy::hwy_step_wide_kernel<2, 2>"
    assert vu.launched(v0, dict(vu.BLOCK), 3)[0] == "hwy::hwy_step_kernel<1, 3>" and vu.step_shape(v0, dict(vu.BLOCK)) == 0
    assert vu.step_shape(dict(v0, vehicles_count=63), {}) == 3 and vu.step_shape(dict(v0, vehicles_count=64), {"tuning": {"block_kernel": 1}}) == 0
    assert vu.step_shape(dict(v0, other_vehicles_type=vu.LINEAR), {}) == 0 and vu.step_shape(dict(v0, **vu.DIRECT), {}) == 0
    # hwy_create's own choice: 3 / 4 on the two sides of 3 wavefronts per SIMD of a 256-CU part
    lin = dict(d, vehicles_count=100, other_vehicles_type=vu.LINEAR)
    assert vu.default_waves_per_eu(lin, {}, 1536) == 3 and vu.default_waves_per_eu(lin, {}, 1537) == 4


# --------------------------------------------------------------------------- 2. every build against the default build

def _cases():
    out = []
    for label, d, kw in ROWS:
        n = _abi.make_config(d, 1, **kw).num_vehicles
        if n < 256:  # (the emulation of 256 vehicles takes seconds and has nothing of its own to show: one build)
            out.append(pytest.param("emu", label, d, kw, id=f"emu-{ident(label)}"))
        out.append(pytest.param("hip", label, d, kw, id=f"hip-{ident(label)}", marks=pytest.mark.gpu))
    return out


@pytest.mark.parametrize("backend,label,d,kw", _cases())
def test_every_build_equals_the_default_build(backend, label, d, kw):
    """One engine per waves_per_eu value against the untuned one: the same device reset and auto-reset, the same random actions,
    K calls of step() and one rollout() of K more -- EQUAL after every step and in the final state.  Episodes last 3 steps, so
    every environment ends and is re-spawned inside the run, in every build."""
    n = _abi.make_config(d, 1, **kw).num_vehicles
    assert vu.label_shape(label) == vu.step_shape(d, kw), f"{label}: its step() runs shape {vu.step_shape(d, kw)}"
    if backend == "emu":
        E, K, vals = 2, 2, (4,)
    else:
        E, K, vals = (4 if n >= 129 else 8), 6, vu.values(kw)
    n_done = vu.compare_row(backend, d, kw, {f"waves_per_eu={v}": {"waves_per_eu": v} for v in vals}, E, K)
    assert n_done >= E, f"{label}: only {n_done} episodes ended in {2 * K} steps of {E} environments"


def _two_small_engines(seeds_b, base_seed_b):
    label, d, kw = ROWS[0]
    d = dict(d, vehicles_count=11, simulation_frequency=5)
    a, b = vu.make_engine("emu", d, kw, 2), vu.make_engine("emu", d, vu.with_tuning(kw, waves_per_eu=4), 2)
    vu.reset_for_comparison(a, d, [5, 6], base_seed=9)
    vu.reset_for_comparison(b, d, seeds_b, base_seed=base_seed_b)
    return a, b


def test_the_comparison_raises_on_engines_reset_with_different_seeds():
    """The comparison of part 2 compares something: two engines that were NOT reset alike fail it -- with different seeds at once,
    with different auto-reset streams once the first episodes have ended -- and the same two reset alike pass it."""
    a, b = _two_small_engines([5, 6], 9)
    assert vu.assert_builds_identical(a, {"same": b}, K=2) >= 2
    a, b = _two_small_engines([5, 7], 9)
    with pytest.raises(AssertionError, match="after the reset"):
        vu.assert_builds_identical(a, {"other seeds": b}, K=2)
    a, b = _two_small_engines([5, 6], 10)
    with pytest.raises(AssertionError, match="other stream: (step|rollout)"):
        vu.assert_builds_identical(a, {"other stream": b}, K=2)
    with pytest.raises(AssertionError, match="nothing to compare"):
        vu.assert_builds_identical(a, {}, K=2)


def test_the_comparison_raises_when_the_table_names_another_kernel(monkeypatch):
    """The shape assertion of the comparison is live: highway-v0 on 4 lanes runs the kernel compiled for it on every step(); a
    table that says "the generic kernel" for it (the state of this file before the shapes had rows) fails on the first step."""
    def pair():
        d = dict(vu.hwy(12), simulation_frequency=15)
        a, b = vu.make_engine("emu", d, {}, 2), vu.make_engine("emu", d, vu.with_tuning({}, waves_per_eu=4), 2)
        for eng in (a, b):
            vu.reset_for_comparison(eng, d, [5, 6], base_seed=9)
        return a, b
    assert vu.step_shape(dict(vu.hwy(12), simulation_frequency=15), {}) == 3
    a, b = pair()
    assert vu.assert_builds_identical(a, {"same": b}, K=3) >= 2
    monkeypatch.setattr(vu, "step_shape_of_config", lambda c: 0)
    a, b = pair()
    with pytest.raises(AssertionError, match="default: step 0: the launch ran shape 3"):
        vu.assert_builds_identical(a, {"same": b}, K=3)


# Builds no test has executed, against the ORACLE (free running, tests/families_util.py: rollout, its tolerances): this does not
# rest on the default build.  {"waves_per_eu": 4, "block_kernel": 1} at N = 65 are the workgroup builds that spill.
FAMILY_CONFIGS = {
    "idm": {},
    "linear": {"other_vehicles_type": vu.LINEAR},
    "direct": dict(vu.DIRECT),
}


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(FAMILY_CONFIGS))
@pytest.mark.parametrize("total,fast,tuning", [(65, True, {"waves_per_eu": 4, "block_kernel": 1}), (64, False, {"waves_per_eu": 1})],
                         ids=["block-N65-wpe4", "wave-N64-wpe1"])
def test_unexecuted_builds_against_the_oracle(family, total, fast, tuning):
    cfg = _abi.highway_fast_default_config()
    cfg.update({"vehicles_count": total - 1, "lanes_count": 4, "tuning": tuning}, **FAMILY_CONFIGS[family])
    rollout("hip", cfg, fast, E=8, steps=8, seed=20 + total)


@pytest.mark.gpu
def test_merge_two_wave_build_against_the_oracle():
    from tests.test_net_parity import _rollout_vs_oracle
    cfg = merge.merge_generic_default_config()
    cfg.update({"lanes_count": 3, "vehicles_count": 20, "controlled_vehicles": 2, "tuning": {"waves_per_eu": 2},
                "action": {"type": "MultiAgentAction", "action_config": {"type": "DiscreteMetaAction"}},
                "observation": {"type": "MultiAgentObservation", "observation_config": {"type": "Kinematics"}}})
    _rollout_vs_oracle("hip", cfg, "merge-generic", E=8, steps=12, seed=3)


# --------------------------------------------------------------------------- 3. the engine's own choice above the threshold

@pytest.mark.gpu
@pytest.mark.parametrize("label,d,E", [
    ("linear N=101", vu.hwy(101, other_vehicles_type=vu.LINEAR), 2048),
    ("idm OccupancyGrid N=200", vu.hwy(200, **vu.GRID), 1024),
], ids=["linear-N101-E2048", "idm-grid-N200-E1024"])
def test_the_engines_own_choice_above_the_threshold(label, d, E):
    """The smallest batches with num_envs x ceil(N / 64) > 3 x 4 x CUs for any part up to 304 CUs (4096 wavefronts > 3648): the
    untuned engine takes the 4-wave workgroup build there.  Untuned, waves_per_eu=3 and waves_per_eu=4 are EQUAL -- whichever
    build the engine took is held to the one the suite verifies."""
    nw = (_abi.make_config(d, 1).num_vehicles + 63) // 64
    assert E * nw > 3 * 4 * 304 and vu.launched(d, {}, 4)[0] in ("hwy::hwy_step_linear_kernel<2, 4>", "hwy::hwy_step_kernel<4, 4>")
    n_done = vu.compare_row("hip", d, {}, {"waves_per_eu=3": {"waves_per_eu": 3}, "waves_per_eu=4": {"waves_per_eu": 4}}, E, K=4)
    assert n_done >= E


# --------------------------------------------------------------------------- 4. tune_extra_lds

@pytest.mark.gpu
@pytest.mark.parametrize("label,d,kw", [
    ("idm ego-only", vu.hwy(50), {"fast": True}),
    ("idm full-scan V0Shape4", vu.hwy(50), {}),
    ("idm full-scan generic", vu.hwy(50, lanes_count=5), {}),
    ("idm FastShape4", vu.fast(50, 4), {"fast": True}),
    ("linear", vu.hwy(50, other_vehicles_type=vu.LINEAR), {}),
    ("direct", vu.hwy(50, **vu.DIRECT), {}),
], ids=["idm-ego-only", "idm-full-scan", "idm-full-scan-generic", "idm-fast-shape", "linear", "direct"])
def test_extra_lds_changes_nothing(label, d, kw):
    """Dynamic LDS on the one-wavefront launches (fewer resident wavefronts per SIMD) against none: 8 KB and 32 KB, both under
    64 KB per workgroup with the kernels' static share (under 10 KB, tests/test_kernel_resources.py).  idm-full-scan is highway-v0
    on 4 lanes, whose step() runs the kernel compiled for it (V0Shape4); idm-full-scan-generic (5 lanes) is the generic full-scan
    kernel and idm-fast-shape the kernel of highway-fast-v0 on 4 lanes."""
    assert vu.label_shape(label) == vu.step_shape(d, kw), label
    n_done = vu.compare_row("hip", d, kw, {f"extra_lds={v}": {"extra_lds": v} for v in (8192, 32768)}, E=8, K=6)
    assert n_done >= 8
