"""Shared helpers of the Lidar door's tests: the fixtures of tests/golden/lidar_door (make_golden_lidar_door.py's records, loaded by
the family's own loader of tests/golden_util.py / tests/lidar_util.py), the backends (``emu`` = tests/emu/emu_lidar_door.py on the
CPU, ``hip`` = the engine on the MI355X) and the comparison criterion, which is tests/lidar_util.py's: float32, same shape, every
value finite, ZERO cells off by more than ``OBS_ATOL`` = 1e-6."""
from __future__ import annotations

import json
import os

import numpy as np

from highwayenv_amd import _abi
from tests.backends import BACKENDS  # noqa: F401  (re-exported)
from tests.golden_util import GoldenIntersection, GoldenMerge, ix_engine_state
from tests.lidar_util import OBS_ATOL, LidarGolden, cells_off  # noqa: F401  (re-exported)

DOOR_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lidar_door")
MERGE = ["door_merge", "door_merge_generic_ma4", "door_merge_v1", "door_crafted"]
IX = ["door_ix", "door_ix_ma3"]
CELLS = "door_cells"
FIXTURES = MERGE + IX + [CELLS]
CELLS_EXTRA = (1, 65, 256)


def make_engine(backend: str, cfg):
    if backend == "emu":
        from tests.emu.emu_lidar_door import LidarDoorEmuEngine
        return LidarDoorEmuEngine(cfg)
    from highwayenv_amd.engine import Engine
    return Engine(cfg)


def env_class(backend: str, base):
    """`base` (a Batched*Env or a drop-in) on the backend: the emulation's engine has the door's entry points."""
    if backend != "emu":
        return base
    from tests.emu.emu_lidar_door import LidarDoorEmuEngine
    return type("Emu" + base.__name__, (base,), {"_engine_factory": staticmethod(lambda cfg, device, stream: LidarDoorEmuEngine(cfg))})


def arrays(name: str) -> dict:
    with np.load(os.path.join(DOOR_DIR, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def params_of(data: dict, cells=None) -> _abi.HwyLidarParams:
    p = json.loads(str(data["lidar_json"]))
    return _abi.lidar_door_params(p["cells"] if cells is None else cells, p["maximum_range"], p["normalize"])


def _kinematics(A: int, inner=None) -> dict:
    inner = inner or {"type": "Kinematics"}
    return inner if A == 1 else {"type": "MultiAgentObservation", "observation_config": inner}


def assert_same(got, want, what: str):
    """The criterion: float32, the reference's shape, finite, zero cells off by more than OBS_ATOL."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == np.shape(want), (what, got.dtype, got.shape, np.shape(want))
    assert np.isfinite(got).all(), f"{what}: a value is not finite"
    off = cells_off(got, want)
    assert off == 0, f"{what}: {off} cells differ by more than {OBS_ATOL}"


class DoorCase:
    """One fixture as (config of an engine with a KINEMATICS observation for all recorded states at once, the states, the
    parameters, the reference's observations [S * E, A, cells, 2] in the same order, labels)."""

    def __init__(self, name: str):
        self.name = name
        data = self.data = arrays(name)
        self.params = [params_of(data)] if name != CELLS else [params_of(data, c) for c in CELLS_EXTRA]
        if name in MERGE:
            g = self.g = GoldenMerge(name, data)
            g.config["observation"] = _kinematics(g.A)
            sts = [g.state("init")] + [g.state("step", t) for t in range(g.steps)]
            self.want = [np.concatenate([data["obs0"]] + [data["obs"][t] for t in range(g.steps)])]
            self.cfg = g.hwy_config(len(sts) * g.E)
            self.state = {k: np.concatenate([s[k] for s in sts]) for k in sts[0]}
        elif name in IX:
            from highwayenv_amd import intersection
            g = self.g = GoldenIntersection(name, data)
            g.config["observation"] = _kinematics(g.A, intersection.intersection_default_config()["observation"])
            sts = []
            for t in range(-1, g.steps):
                s = g.state("init") if t < 0 else g.state("next", t)
                s["road_steps"][...] = data["road_steps0"] if t < 0 else data["next_road_steps"][t]
                s["time"][...] = float(t + 1)
                sts.append(s)
            # the yardstick after a step: observe() called AFTER step() (the list after _clear_vehicles / _spawn_vehicle)
            self.want = [np.concatenate([data["obs0"]] + [data["observe"][t] for t in range(g.steps)])]
            cfg_d = dict(g.config, max_vehicles=g.N, host_traffic=True)
            self.cfg = _abi.make_config(cfg_d, len(sts) * g.E, scenario="intersection")
            self.state = ix_engine_state(g, {k: np.concatenate([s[k] for s in sts]) for k in sts[0]}, self.cfg)
        else:
            g = self.g = LidarGolden(name, data)
            g.config["observation"] = {"type": "Kinematics"}
            sts = [g.state("init")] + [g.state("step", t) for t in range(g.steps)]
            self.want = [np.concatenate([data[f"obs0_c{c}"]] + [data[f"obs_c{c}"][t] for t in range(g.steps)]) for c in CELLS_EXTRA]
            self.cfg = g.hwy_config(len(sts) * g.E)
            self.state = {k: np.concatenate([s[k] for s in sts]) for k in sts[0]}
        self.E, self.S = g.E, len(sts)
        assert self.cfg.obs_type == _abi.OBS_KINEMATICS

    def engine(self, backend: str):
        eng = make_engine(backend, self.cfg)
        eng.set_state(self.state)
        return eng

    def check(self, eng, what: str = ""):
        for p, want in zip(self.params, self.want):
            assert_same(eng.lidar_observe(p), want, f"{self.name} cells={p.cells} {what}")
