"""The one-wavefront step kernel compiled for a registered configuration (csrc/hwy_wave.h: FixedShape; csrc/hwy_kernels_shapes.hip)
against the generic kernel, and the rule that picks between them (csrc/hwy_launch_family.h: step_shape_of).

1. Bit-identity: an engine whose launches take the shape kernel and one held to the generic kernel (hwy_step_shapes) take the same
   random actions through 12 policy steps with device spawn and auto-reset, in dense traffic; every output plane and the whole
   state are EQUAL after every step, with and without a block order -- at 12 vehicles, at the edges of N (1, 2, 5, 64), on the
   MI355X in every register-allocation build at N = 64, and through the HighwayVectorEnv front end in both autoreset modes.  The run is only accepted if the GENERIC engine's own
   trajectory shows what the specialised code could get wrong: an ego crash (SAT and impact), an auto-reset, an observation with
   zeroed rows, FASTER at the top and SLOWER at the bottom of the speed ladder, LANE_LEFT on lane 0, a vehicle on two lanes.
2. Selection: every field a shape fixes, flipped one at a time, sends the launch to the generic kernel (hwy_last_step_shape == 0)
   with the forced-generic engine's results; the registered configurations themselves report their shape.

Both run on the CPU emulation, whose launch layer is the product's and whose shape kernels CHECK what the device build assumes (a
launch that breaks a shape's promise traps), and on the MI355X under -m gpu."""
import ctypes as C

import numpy as np
import pytest

from highwayenv_amd import _abi
from tests.backends import BACKENDS, make_engine

FASTER, SLOWER, LANE_LEFT = 3, 4, 0  # ids of the five-action table (hwy_engine.h: HWY_ACTIONS_ALL)
E, N_OTHERS, STEPS = 8, 11, 12       # 8 environments x 12 vehicles, 12 policy steps
DENSITY = 2.0


def _library(backend):
    """The library whose launch layer runs: both carry hwy_step_shapes / hwy_last_step_shape (csrc/hwy_launch_family.h)."""
    if backend == "emu":
        from tests.emu import emu
        return emu.lib()
    from highwayenv_amd import _lib
    return _lib.load()


@pytest.fixture
def shapes(backend):
    """set(on) / last(); the process-wide setting is put back afterwards."""
    lib = _library(backend)
    was = lib.hwy_step_shapes(C.c_int(-1))

    class Switch:
        @staticmethod
        def set(on):
            lib.hwy_step_shapes(C.c_int(int(on)))

        @staticmethod
        def last():
            return lib.hwy_last_step_shape()
    yield Switch
    lib.hwy_step_shapes(C.c_int(was))


def _config(kind, **over):
    """The dict and the make_config keywords of a registered configuration at the test's size."""
    fast = kind != "v0-4"
    d = _abi.highway_fast_default_config() if fast else _abi.highway_default_config()
    d.update({"vehicles_count": N_OTHERS, "lanes_count": 3 if kind == "fast-3" else 4, "vehicles_density": DENSITY})
    d.update(over)
    return d, fast


SHAPES = {"fast-3": 1, "fast-4": 2, "v0-4": 3}
# seeds (reset, auto-reset stream, actions) for which the generic kernel's run shows all six events: found on the CPU emulation
SEEDS = {"fast-3": (59, 70, 61), "fast-4": (28, 39, 30), "v0-4": (28, 39, 30)}


def _fresh(backend, d, fast, seeds):
    eng = make_engine(backend, _abi.make_config(d, E, fast=fast))
    eng.reset(seeds=1000 * seeds[0] + np.arange(E, dtype=np.uint64), vehicles_density=DENSITY)
    eng.set_autoreset(True, base_seed=seeds[1], vehicles_density=DENSITY)
    return eng


def _assert_same(got, want, what):
    for name, a, b in zip(("obs", "reward", "terminated", "truncated"), got[:4], want[:4]):
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: {name}")
    for k in ("speed", "crashed"):
        np.testing.assert_array_equal(got[4][k], want[4][k], err_msg=f"{what}: info {k}")


def _assert_same_state(a, b, what):
    sa, sb = a.get_state(), b.get_state()
    assert set(sa) == set(sb)
    for f in sa:
        np.testing.assert_array_equal(sa[f], sb[f], err_msg=f"{what}: state {f}")
    return sb


def events_of_step(before, acts, done_before, out, after, lanes):
    """Which of the six events one policy step of the GENERIC engine shows.  before / after: get_state() around it; done_before: the
    environments this step re-spawned instead of stepping."""
    obs, _, term, trunc, info = out
    live = ~done_before
    a = acts[:, 0]
    v = before["speed"][:, 0]
    rung = np.clip(np.rint((v - 20.0) / 10.0 * 2), 0, 2)  # MDPVehicle.speed_to_index on the default ladder (controller.py:259-284)
    y = np.concatenate([before["y"], after["y"]])
    two = np.zeros(y.shape, bool)
    for lane in range(lanes - 1):  # on_lane with margin 1: |y - 4 lane| <= 3 for two neighbouring lanes
        two |= (np.abs(y - 4.0 * lane) <= 3.0) & (np.abs(y - 4.0 * (lane + 1)) <= 3.0)
    return {
        "ego crash": bool((info["crashed"][:, 0] & live).any()),
        "auto-reset": bool(done_before.any() and (after["time"][done_before] == 0).all()),
        "zeroed rows": bool((obs[live][:, 0, 1:, 0] == 0).any()),
        "FASTER at the top": bool((live & (a == FASTER) & (rung == 2)).any()),
        "SLOWER at the bottom": bool((live & (a == SLOWER) & (rung == 0)).any()),
        "LANE_LEFT on lane 0": bool((live & (a == LANE_LEFT) & (before["target_lane"][:, 0] == 0)).any()),
        "two lanes at once": bool(two.any()),
    }


def _run_against_generic(backend, kind, seeds, block_order, shapes, **over):
    """STEPS policy steps of an engine on the shape kernel and of one held to the generic kernel, EQUAL after every step; returns
    which events the generic engine's trajectory showed (events_of_step)."""
    d, fast = _config(kind, **over)
    spec, gen = _fresh(backend, d, fast, seeds), _fresh(backend, d, fast, seeds)
    rng = np.random.default_rng(seeds[2])
    if block_order:
        spec.set_block_order(np.random.default_rng(1).permutation(E))
    seen = {}
    before = _assert_same_state(spec, gen, "after the reset")
    done = np.zeros(E, bool)
    try:
        for t in range(STEPS):
            acts = rng.integers(0, 5, size=(E, 1)).astype(np.int32)
            shapes.set(True)
            got = spec.step(acts)
            assert shapes.last() == SHAPES[kind], f"step {t}: the specialised engine ran shape {shapes.last()}"
            shapes.set(False)
            want = gen.step(acts)
            assert shapes.last() == 0, f"step {t}: the forced-generic engine ran shape {shapes.last()}"
            _assert_same(got, want, f"step {t}")
            after = _assert_same_state(spec, gen, f"step {t}")
            for name, hit in events_of_step(before, acts, done, want, after, d["lanes_count"]).items():
                seen[name] = seen.get(name, False) or hit
            before, done = after, want[2] | want[3]
    finally:
        spec.close()
        gen.close()
    return seen


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("block_order", [False, True], ids=["identity", "block-order"])
@pytest.mark.parametrize("kind", list(SHAPES))
def test_shape_kernel_equals_generic_kernel(backend, kind, block_order, shapes):
    seen = _run_against_generic(backend, kind, SEEDS[kind], block_order, shapes)
    assert all(seen.values()), f"the run does not exercise: {[k for k, v in seen.items() if not v]}"


# The edges of N: the ego alone (every other observation row zeroed), fewer vehicles than the 5 observation rows, exactly as many,
# and a wavefront without an idle lane.  Episodes of 3 policy steps: whatever the traffic does, every environment is truncated and
# re-spawned by the kernel within the 12 steps -- the one event required here (the six of N = 12 need traffic to happen in).
EDGE_SIZES = (1, 2, 5, 64)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("block_order", [False, True], ids=["identity", "block-order"])
@pytest.mark.parametrize("n", EDGE_SIZES, ids=[f"N{n}" for n in EDGE_SIZES])
@pytest.mark.parametrize("kind", list(SHAPES))
def test_shape_kernel_equals_generic_kernel_at_the_edges_of_n(backend, kind, n, block_order, shapes):
    seen = _run_against_generic(backend, kind, (7 + n, 8 + n, 9 + n), block_order, shapes, vehicles_count=n - 1, duration=3)
    assert seen["auto-reset"], "no environment was re-spawned within the run"


@pytest.mark.parametrize("backend", [pytest.param("hip", id="hip", marks=pytest.mark.gpu)])
@pytest.mark.parametrize("w", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", list(SHAPES))
def test_every_build_of_a_shape_kernel_equals_the_generic_build(backend, kind, w, shapes):
    """hwy_shape_wave_kernel<shape, w> against hwy_step_wave_kernel<w, ...>, w = waves per SIMD the register allocator leaves room
    for: 64 vehicles, no idle lane.  (The emulation compiles one build: nothing of its own to show.)"""
    seen = _run_against_generic(backend, kind, (71, 72, 73), False, shapes, vehicles_count=63, duration=3, tuning={"waves_per_eu": w})
    assert seen["auto-reset"], "no environment was re-spawned within the run"


# --------------------------------------------------------------------------- the front end

FRONT_ENDS = {"highway-fast-v0": ({}, 1), "highway-fast-v0, 4 lanes": ({"lanes_count": 4}, 2), "highway-v0": ({}, 3)}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("mode", ["NextStep", "SameStep"])
@pytest.mark.parametrize("which", list(FRONT_ENDS), ids=["fast", "fast-4", "v0"])
def test_the_vector_front_end_computes_the_same_with_shapes_on_and_off(backend, which, mode, shapes):
    """HighwayVectorEnv over the registered ids, numpy outputs: 8 steps with the shape kernels allowed equal the same 8 steps with
    every launch held to the generic kernel -- observation, reward, terminated, truncated, the info planes and, in SameStep
    mode, the terminal observations.  NextStep is the device's auto-reset, so every step() runs the shape's kernel.  SameStep
    steps WITHOUT the device's auto-reset (ended environments are re-spawned by a masked reset behind the step), so its launches
    match no shape and run the generic kernel whatever the switch says: hwy_last_step_shape() == 0."""
    from highwayenv_amd import envs, vector
    from tests.backends import env_class
    over, shape = FRONT_ENDS[which]
    cls = env_class(backend, envs.batched_class(which.split(",")[0]))
    config = {"vehicles_count": N_OTHERS, "duration": 3, **over}
    runs = []
    for on in (True, False):
        shapes.set(on)
        venv = vector.HighwayVectorEnv(cls, num_envs=E, config=config, autoreset_mode=mode)
        try:
            obs, infos = venv.reset(seed=21)
            trace = [(obs, infos["speed"], infos["crashed"])]
            rng = np.random.default_rng(22)
            for t in range(8):
                obs, reward, term, trunc, infos = venv.step(rng.integers(0, 5, size=E))
                assert shapes.last() == (shape if on and mode == "NextStep" else 0), f"{which} {mode}, shapes {on}, step {t}: shape {shapes.last()}"
                final = [None if o is None else np.array(o) for o in infos["final_obs"]] if "final_obs" in infos else None
                trace.append((np.array(obs), np.array(reward), np.array(term), np.array(trunc), np.array(infos["speed"]),
                              np.array(infos["crashed"]), final))
        finally:
            venv.close()
        runs.append(trace)
    n_done = n_final = 0
    for t, (a, b) in enumerate(zip(*runs)):
        for x, y in zip(a[:6], b[:6]):
            np.testing.assert_array_equal(x, y, err_msg=f"{which} {mode}: call {t}")
        if t > 0:
            n_done += int((a[2] | a[3]).sum())
            assert (a[6] is None) == (b[6] is None)
            for fa, fb in zip(a[6] or [], b[6] or []):
                assert (fa is None) == (fb is None)
                if fa is not None:
                    n_final += 1
                    np.testing.assert_array_equal(fa, fb, err_msg=f"{which} {mode}: final_obs of call {t}")
    assert n_done >= E and (n_final == n_done if mode == "SameStep" else n_final == 0), (n_done, n_final)


# --------------------------------------------------------------------------- selection

def _emu_full_step(eng, acts, info=True):
    """A full policy step of the emulated engine with the action plane and / or the info planes unbound (tests/emu/emu.py: _run
    always binds them)."""
    from tests.emu import emu
    L = emu.lib()
    p = emu._p
    obs = np.zeros((eng.E, eng.A, *_abi.obs_shape(eng.cfg)), np.float32)
    reward, term, trunc = np.zeros((eng.E, eng.A)), np.zeros(eng.E, np.uint8), np.zeros(eng.E, np.uint8)
    speed, crashed = (np.zeros((eng.E, eng.A)), np.zeros((eng.E, eng.A), np.uint8)) if info else (None, None)
    s = _abi.state_struct(eng.st)
    ar = eng.autoreset
    L.emu_set_shadow(None, None, None, None)
    L.emu_set_block_order(None)
    rc = L.emu_run(C.byref(eng.cfg), C.byref(s), p(eng.done, C.c_uint8), p(eng.episode, C.c_uint32), C.c_int(1),
                   C.c_int(eng.cfg.frames_per_step), p(acts, C.c_int32), p(obs, C.c_float), p(reward, C.c_double), p(term, C.c_uint8),
                   p(trunc, C.c_uint8), p(speed, C.c_double), p(crashed, C.c_uint8), C.c_int(ar[0]), C.c_uint64(ar[1]),
                   C.c_double(ar[2]), C.c_double(ar[3]), C.c_int(ar[4]))
    assert rc == 0
    return obs, reward, term.astype(bool), trunc.astype(bool), {"speed": reward * 0 if speed is None else speed,
                                                                "crashed": term * 0 if crashed is None else crashed}


def _hip_step_without_info(eng, acts):
    """hwy_step_device on device planes with both info pointers NULL (hwy_step always binds the engine's own)."""
    import torch
    dev = torch.device("cuda")
    a = torch.as_tensor(acts, device=dev).contiguous()
    obs = torch.zeros((eng.E, eng.A, *_abi.obs_shape(eng.cfg)), dtype=torch.float32, device=dev)
    reward = torch.zeros((eng.E, eng.A), dtype=torch.float64, device=dev)
    term, trunc = torch.zeros(eng.E, dtype=torch.uint8, device=dev), torch.zeros(eng.E, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    eng.step_device(a.data_ptr(), obs.data_ptr(), reward.data_ptr(), term.data_ptr(), trunc.data_ptr())
    eng.sync()
    reward = reward.cpu().numpy()
    return obs.cpu().numpy(), reward, term.cpu().numpy().astype(bool), trunc.cpu().numpy().astype(bool), {"speed": reward * 0,
                                                                                                         "crashed": reward * 0}


def _full_step(eng, acts):
    return eng.step(acts)


def _frames_only(eng, acts):
    eng.step_frames(acts, eng.cfg.frames_per_step)


def _without_actions(backend):
    # the product's C ABI takes a NULL action plane in hwy_step_frames only (hwy_step / hwy_step_device refuse it); the emulation's
    # driver binds whatever it is given, so there the launch is a full step without actions
    if backend == "emu":
        return lambda eng, acts: _emu_full_step(eng, None)
    return lambda eng, acts: eng.step_frames(None, eng.cfg.frames_per_step)


def _without_info(backend):
    if backend == "emu":
        return lambda eng, acts: _emu_full_step(eng, np.ascontiguousarray(acts, np.int32), info=False)
    return _hip_step_without_info


LONGI = {"action": {"type": "DiscreteMetaAction", "lateral": False}}
# (label, config overrides, auto-reset, the call): ONE field of what FixedShape fixes differs from highway-fast-v0 on 4 lanes
FLIPS = [
    ("L=2", {"lanes_count": 2}, True, None),
    ("A=2", {"controlled_vehicles": 2, "vehicles_count": N_OTHERS - 1}, True, None),
    ("V=7", {"observation": {"type": "Kinematics", "vehicles_count": 7}}, True, None),
    ("see_behind", {"observation": {"type": "Kinematics", "see_behind": True}}, True, None),
    ("absolute", {"observation": {"type": "Kinematics", "absolute": True}}, True, None),
    ("action table LONGI", LONGI, True, None),
    ("T=3", {"simulation_frequency": 3}, True, None),
    ("four target speeds", {"action": {"type": "DiscreteMetaAction", "target_speeds": [15, 20, 25, 30]}}, True, None),
    ("no info planes", {}, True, "without_info"),
    ("full_step=0", {}, True, "frames_only"),
    ("auto-reset off", {}, False, None),
    ("actions=nullptr", {}, True, "without_actions"),
]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("label,over,autoreset,call", FLIPS, ids=[f[0].replace(" ", "-") for f in FLIPS])
def test_any_flipped_field_runs_the_generic_kernel(backend, label, over, autoreset, call, shapes):
    d, fast = _config("fast-4", **over)
    cfg = _abi.make_config(d, E, fast=fast)
    step = {None: _full_step, "frames_only": _frames_only, "without_actions": _without_actions(backend),
            "without_info": _without_info(backend)}[call]
    a, b = make_engine(backend, cfg), make_engine(backend, cfg)
    try:
        for eng in (a, b):
            eng.reset(seeds=7000 + np.arange(E, dtype=np.uint64), vehicles_density=DENSITY)
            if autoreset:
                eng.set_autoreset(True, base_seed=5, vehicles_density=DENSITY)
        rng = np.random.default_rng(6)
        for t in range(3):
            acts = rng.integers(0, _abi.num_actions(cfg), size=(E, cfg.num_agents)).astype(np.int32)
            shapes.set(True)
            got = step(a, acts)
            assert shapes.last() == 0, f"{label}, step {t}: shape {shapes.last()} took a launch it does not describe"
            shapes.set(False)
            want = step(b, acts)
            assert shapes.last() == 0
            if got is not None:
                _assert_same(got, want, f"{label}, step {t}")
            _assert_same_state(a, b, f"{label}, step {t}")
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind,d,fast,shape", [
    ("highway-fast-v0", _abi.highway_fast_default_config(), True, 1),
    ("highway-fast-v0, 4 lanes x 51 vehicles", dict(_abi.highway_fast_default_config(), lanes_count=4, vehicles_count=50), True, 2),
    ("highway-v0", _abi.highway_default_config(), False, 3),
], ids=["fast", "fast-4x51", "v0"])
def test_the_registered_configurations_report_their_shape(backend, kind, d, fast, shape, shapes):
    """The package's defaults, exactly: a full step with auto-reset runs the shape's kernel, the same step with shapes off or
    before hwy_set_autoreset the generic one, and a multi-step launch the generic rollout kernel."""
    eng = make_engine(backend, _abi.make_config(d, 2, fast=fast))
    try:
        eng.reset(seeds=np.arange(2, dtype=np.uint64))
        acts = np.ones((2, 1), np.int32)
        shapes.set(True)
        eng.step(acts)
        assert shapes.last() == 0, f"{kind}: before hwy_set_autoreset"
        eng.set_autoreset(True, base_seed=1)
        eng.step(acts)
        assert shapes.last() == shape, kind
        eng.rollout(np.ones((2, 2, 1), np.int32))
        assert shapes.last() == 0, f"{kind}: rollout"
        eng.step(acts)
        assert shapes.last() == shape, kind
        shapes.set(False)
        eng.step(acts)
        assert shapes.last() == 0, f"{kind}: shapes off"
    finally:
        eng.close()
