"""The act kernel (csrc/hwy_act.h: hwy_act_continuous_kernel) against a NumPy restatement of ``ContinuousAction.get_action`` for a
float32 action (tests/continuous_util.py: restate), bit for bit, on the CPU emulation of the kernel source (``emu``) and on the
MI355X (``hip``) -- and the restatement itself against ``utils.lmap`` of the unmodified reference where that is installed."""
import numpy as np
import pytest

from highwayenv_amd import _abi, build
from oracle import ref_stub
from tests.continuous_util import BACKENDS, make_engine, restate, restate_axis

F32 = np.float32
EDGES = np.array([1.0, -1.0, 0.0, -0.0, np.nextafter(F32(1), F32(0)), np.nextafter(F32(1), F32(2)), np.nextafter(F32(-1), F32(0)),
                  np.nextafter(F32(-1), F32(-2)), 1e-30, -1e-30, 1.3, -1.3, 7.5, -1e9, 0.5, -0.25, 1 / 3], F32)
#: the default ranges, an asymmetric pair whose ends are not float32 numbers, and +-pi/3 (the widest steering the engine takes)
RANGES = [((-5, 5.0), (-np.pi / 4, np.pi / 4)), ((-3.3, 2.1), (-0.3, 0.1)), ((-1e-3, 123.456), (-np.pi / 3, np.pi / 3))]


def _cfg(E, A):
    d = _abi.highway_fast_default_config()
    act = {"type": "DiscreteAction", "steering_range": [-0.05, 0.05]}
    d.update({"vehicles_count": 5, "lanes_count": 3, "controlled_vehicles": A,
              "action": act if A == 1 else {"type": "MultiAgentAction", "action_config": act}})
    if A > 1:
        d["observation"] = {"type": "MultiAgentObservation", "observation_config": {"type": "Kinematics"}}
    return _abi.make_config(d, E, fast=True)


def _params(ranges, longitudinal=True, lateral=True):
    return _abi.continuous_params({"type": "ContinuousAction", "acceleration_range": list(ranges[0]), "steering_range": list(ranges[1]),
                                   "longitudinal": longitudinal, "lateral": lateral})


def _rows(rng, n, size):
    """n rows of `size` components: every pair of edge values first, then uniform draws from [-1.3, 1.3]."""
    edge = np.stack(np.meshgrid(EDGES, EDGES, indexing="ij"), -1).reshape(-1, 2)[:, :size]
    rest = rng.uniform(-1.3, 1.3, size=(n - len(edge), size)).astype(F32)
    return np.concatenate([edge, rest])


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("A,axes", [(1, (True, True)), (2, (True, True)), (1, (True, False)), (2, (False, True))])
def test_act_kernel_equals_the_restatement_bit_for_bit(backend, A, axes):
    """5200 environments x A agents (more than one workgroup, a last one that is not full), three range pairs: the stored pair of
    every row is the restatement's double; an axis that is not controlled holds 0.0."""
    E = 5200
    eng = make_engine(backend, _cfg(E, A))
    rng = np.random.default_rng(17 + A)
    for ranges in RANGES:
        p = _params(ranges, *axes)
        acts = _rows(rng, E * A, p.size).reshape(E, A, p.size)
        eng.set_controls(np.full((E, A), 9.0), np.full((E, A), 0.5))
        eng.act_continuous(p, acts)
        accel, steer = eng.get_controls()
        want_accel, want_steer = restate(p, acts)
        np.testing.assert_array_equal(accel.view(np.uint64), want_accel.view(np.uint64), err_msg=f"{ranges}: acceleration")
        np.testing.assert_array_equal(steer.view(np.uint64), want_steer.view(np.uint64), err_msg=f"{ranges}: steering")
        if not axes[0]:
            assert not accel.any()
        if not axes[1]:
            assert not steer.any()
    eng.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_a_non_finite_row_keeps_its_stored_pair_and_the_host_door_raises(backend):
    E, A = 70, 2
    eng = make_engine(backend, _cfg(E, A))
    p = _params(RANGES[1])
    rng = np.random.default_rng(3)
    acts = rng.uniform(-1.3, 1.3, size=(E, A, 2)).astype(F32)
    acts[3, 0, 0], acts[3, 1, 1], acts[40, 1, 0], acts[69, 0, 1] = np.nan, np.inf, -np.inf, np.nan
    stored = (rng.uniform(-2, 2, (E, A)), rng.uniform(-0.2, 0.2, (E, A)))
    eng.set_controls(*stored)
    for call in (eng.act_continuous, eng.step_continuous, lambda q, a: eng.rollout_continuous(q, a[None])):
        with pytest.raises(ValueError):
            call(p, acts)
        for got, want in zip(eng.get_controls(), stored):  # (nothing ran)
            np.testing.assert_array_equal(got, want)
    eng.act_continuous_device(p, acts) if backend == "emu" else _act_device(eng, p, acts)
    want = restate(p, acts, stored)
    bad = ~np.isfinite(acts).all(-1)
    assert bad.sum() == 4
    for got, w, s in zip(eng.get_controls(), want, stored):
        np.testing.assert_array_equal(got, w)
        np.testing.assert_array_equal(got[bad], s[bad])
    eng.close()


def _act_device(eng, p, acts):
    """hwy_act_continuous_device on a torch tensor (the device door does not validate the values)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(acts)).cuda()
    torch.cuda.synchronize()
    eng.act_continuous_device(p, t.data_ptr())
    eng.sync()


@pytest.mark.parametrize("backend", BACKENDS)
def test_what_the_params_reject(backend):
    from highwayenv_amd.engine import EngineError
    eng = make_engine(backend, _cfg(2, 1))
    acts = np.zeros((2, 1, 2), F32)
    for bad in ({"steering_range": (-1.2, 1.2)}, {"acceleration_range": (-np.inf, 1.0)}, {"longitudinal": 0, "lateral": 0}):
        p = _params(RANGES[0])
        for k, v in bad.items():
            if isinstance(v, tuple):
                getattr(p, k)[0], getattr(p, k)[1] = v
            else:
                setattr(p, k, v)
        with pytest.raises(EngineError):
            eng.act_continuous(p, acts[..., :p.size])
    eng.close()
    d = _abi.highway_fast_default_config()
    d.update({"vehicles_count": 5})
    meta = make_engine(backend, _abi.make_config(d, 2, fast=True))  # DiscreteMetaAction: its vehicles store no controls
    with pytest.raises(EngineError):
        meta.step_continuous(_params(RANGES[0]), acts)
    meta.close()


def test_restatement_edge_values():
    """What the restatement is for, without anything to compare it to: the clip, the ends, and that float32 is not float64."""
    y = (-3.3, 2.1)
    out = restate_axis(EDGES, *y)
    assert out[0] == out[5] == restate_axis(F32(1.3), *y) and out[1] == out[7]      # clipped
    assert out[2] == out[3]                                                          # -0.0 + 1 == 0.0 + 1
    assert out[0] == float(F32(F32(-3.3) + F32(F32(2) * F32(2.1 - -3.3)) / F32(2)))
    in_double = y[0] + (np.clip(EDGES.astype(np.float64), -1, 1) + 1) * (y[1] - y[0]) / 2
    assert (out != in_double).any() and np.abs(out - in_double).max() < 1e-6


@pytest.mark.skipif(not ref_stub.reference_available(), reason="needs the reference package")
def test_restatement_equals_the_reference_lmap():
    """20 000 random float32 actions in [-1.3, 1.3] plus the edge values, every range pair: the stepwise form IS
    ``utils.lmap(np.clip(a, -1, 1)[k], [-1, 1], range)`` of the reference, and that is a float32."""
    ref_stub.install()
    from highway_env import utils
    rng = np.random.default_rng(5)
    vals = np.concatenate([EDGES, rng.uniform(-1.3, 1.3, 20000).astype(F32)])
    for ranges in RANGES:
        for y in ranges:
            clipped = np.clip(vals, -1, 1)
            ref = [utils.lmap(clipped[k], [-1, 1], y) for k in range(len(vals))]
            assert all(type(r) is np.float32 for r in ref)
            np.testing.assert_array_equal(np.asarray([float(r) for r in ref]).view(np.uint64), restate_axis(vals, *y).view(np.uint64))


def test_the_act_kernel_is_in_the_library_without_spills_or_lds():
    res = build.kernel_resources()
    names = [k for k in res if "hwy_act_continuous_kernel" in k]
    assert len(names) == 1, names
    r = res[names[0]]
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["lds"] == 0 and r["scratch"] == 0, r
    assert r["workgroup"] == 256
    assert not any(("step" in k or "rollout" in k) and "act" in k for k in names)
