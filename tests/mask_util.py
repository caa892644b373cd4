"""Shared helpers of the action-mask tests: the fixtures of tests/golden/masks (make_golden_masks.py's record), the backends
(``emu`` = tests/emu/emu.py on the CPU, ``hip`` = the engine on the MI355X) and the reference's list order."""
from __future__ import annotations

import json
import os

import numpy as np

from highwayenv_amd import _abi, envs
from tests.backends import BACKENDS, emu_class, make_engine  # noqa: F401  (re-exported)

MASK_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "masks")
FIXTURES = ["mask_fast", "mask_lanes1", "mask_lanes2", "mask_speeds2", "mask_speeds8", "mask_longi", "mask_lat", "mask_ma2",
            "mask_placed", "mask_merge", "mask_merge_generic", "mask_intersection", "mask_intersection_ma"]
# columns of the three action tables (include/hwy_engine.h: hwy_config.action_set)
COLUMNS = {_abi.ACTIONS_SET_ALL: ("LANE_LEFT", "IDLE", "LANE_RIGHT", "FASTER", "SLOWER"),
           _abi.ACTIONS_SET_LONGI: ("SLOWER", "IDLE", "FASTER"), _abi.ACTIONS_SET_LAT: ("LANE_LEFT", "IDLE", "LANE_RIGHT")}
REFERENCE_ORDER = ("IDLE", "LANE_LEFT", "LANE_RIGHT", "FASTER", "SLOWER")   # DiscreteMetaAction.get_available_actions appends so


class MaskGolden:
    """A fixture of tests/golden/masks."""

    def __init__(self, name: str, data: dict | None = None):
        self.name = name
        if data is None:
            with np.load(os.path.join(MASK_DIR, name + ".npz")) as z:
                data = {k: z[k] for k in z.files}
        self.z = dict(data)
        self.E, self.N, self.steps, self.A, self.n_ids = (int(v) for v in self.z["meta"])
        self.env_id = str(self.z["env_id"])
        self.batched = envs.batched_class(self.env_id)
        self.single = envs.REGISTRY[self.env_id][0]
        self.overrides = json.loads(str(self.z["config_json"]))
        self.config = self.batched.default_config()
        self.config.update(self.overrides)
        self.actions = self.z["actions"]

    def hwy_config(self, num_envs=None) -> _abi.HwyConfig:
        return _abi.make_config(self.config, self.E if num_envs is None else num_envs, fast=self.batched.FAST,
                                scenario=self.batched.SCENARIO)

    def indices(self):
        """The recorded states: None (reset) and every step."""
        return [None] + list(range(self.steps))

    def mask(self, index=None) -> np.ndarray:
        """The reference's table bool [E, A, n_ids] at reset (None) or after step `index`."""
        return self.z["mask0"] if index is None else self.z["mask"][index]

    def state(self, index=None, envs=None) -> dict:
        """The engine's SoA dict of a recorded state (every family: the intersection's with empty routes)."""
        z = self.z

        def get(k):
            a = z[("init_" if index is None else "step_") + k]
            a = a if index is None else a[index]
            return a if envs is None else a[envs]

        E = get("x").shape[0]
        ix = self.batched.SCENARIO == "intersection"
        st = _abi.alloc_state_ix(E, self.N) if ix else _abi.alloc_state(E, self.N)
        for k in _abi.STATE_F64:
            st[k][...] = get(k)
        for k in ("lane", "target_lane", "speed_index"):
            st[k][...] = get(k)
        st["flags"][...] = (get("crashed") * _abi.F_CRASHED + get("has_impact") * _abi.F_HAS_IMPACT
                            + get("check_collisions") * _abi.F_CHECK_COLLISIONS + get("controlled") * _abi.F_CONTROLLED
                            + get("obstacle") * _abi.F_OBSTACLE + (1 - get("present")) * _abi.F_ABSENT)
        return st


def generator():
    """tests/golden/masks/make_golden_masks.py as a module (needs the reference package)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_masks", os.path.join(MASK_DIR, "make_golden_masks.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_list(row, action_set: int) -> list:
    """The list the reference returns for one agent's mask row: ids of the available actions in REFERENCE_ORDER."""
    cols = COLUMNS[action_set]
    return [cols.index(name) for name in REFERENCE_ORDER if name in cols and row[cols.index(name)]]
