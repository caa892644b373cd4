"""Shared helpers of the time-to-collision / finite-MDP planner tests: the fixtures of tests/golden/ttc, the backends (``emu`` =
tests/emu/emu.py on the CPU, ``hip`` = the engine on the MI355X), a numpy restatement of the grid vectorised over the vehicles,
and the numpy fixed-point iteration the planner is held to."""
from __future__ import annotations

import os

import numpy as np

from highwayenv_amd import _abi
from tests.backends import BACKENDS, make_engine  # noqa: F401  (re-exported)
from tests.golden_util import Golden

TTC_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ttc")
RUNS = ["ttc_fast", "ttc_lanes1", "ttc_lanes16", "ttc_speeds2", "ttc_speeds8", "ttc_pf5", "ttc_horizon1", "ttc_n64", "ttc_n65",
        "ttc_n130", "ttc_ma2", "ttc_linear", "ttc_crash", "ttc_rewards"]
PASSES = ["ttc_passes65", "ttc_passes130"]  # hand-placed: vehicles within the horizon in the slots either side of a pass of 64
# the kernel's own boundaries (csrc/hwy_ttc.h): the LDS capacity classes either side of 1024 cells, the value sweep either side of
# 64 states, and every limit at once; ttc_states65 and ttc_max end with hand-placed roads (STATE_ROADS: (environment, observer's s))
BOUNDARIES = ["ttc_cells1024", "ttc_cells1025", "ttc_states64", "ttc_states65", "ttc_max"]
STATE_ROADS = {"ttc_states65": [(2, 63), (3, 64)], "ttc_max": [(2, 63), (3, 64), (4, 127)]}
FIXTURES = RUNS + ["ttc_crafted"] + PASSES + BOUNDARIES
KNIFE = 1e-9   # a candidate with |ttc / tq - rint(ttc / tq)| below this may fall into either neighbouring cell
MARGIN = 5.0   # other.LENGTH / 2 + vehicle.LENGTH / 2


class TtcGolden(Golden):
    """A fixture of tests/golden/ttc: make_golden_ttc.py's record."""

    def __init__(self, name: str, data: dict | None = None):
        if data is None:
            with np.load(os.path.join(TTC_DIR, name + ".npz")) as z:
                data = {k: z[k] for k in z.files}
        super().__init__(name, dict(data))
        self.A = int(data["cfg_controlled_vehicles"])
        self.config["controlled_vehicles"] = self.A
        self.config["other_vehicles_type"] = str(data["cfg_other_vehicles_type"])
        self.config["lane_change_reward"] = float(data["cfg_lane_change_reward"])
        self.horizon = float(data["cfg_horizon"])

    def hwy_config(self, num_envs=None) -> _abi.HwyConfig:
        return _abi.make_config(self.config, self.E if num_envs is None else num_envs, fast=self.fast)

    def params(self, gamma: float = 1.0) -> _abi.HwyTtcParams:
        return _abi.ttc_params(self.config, horizon=self.horizon, gamma=gamma)

    def indices(self):
        """The recorded states: None (reset) and every step."""
        return [None] + list(range(self.steps))

    def load(self, eng, index=None):
        eng.set_state(self.state("init" if index is None else "step", index))
        if eng.cfg.traffic_model == _abi.TRAFFIC_LINEAR:
            eng.set_behavior(self.z["init_behavior"])

    def get(self, key: str, index=None) -> np.ndarray:
        """``grid`` [E, A, V, L, T]; ``transition`` / ``reward`` [E, S, 5], ``terminal`` [E, S], ``state`` [E] (single-agent
        fixtures): the reference's record at reset (None) or after step `index`."""
        return self.z[key + "0"] if index is None else self.z[key][index]

    @property
    def has_tables(self) -> bool:
        return "transition0" in self.z.files


def restate_grid(cfg: _abi.HwyConfig, st: dict, params: _abi.HwyTtcParams):
    """The time-to-collision grid of every (environment, agent) of a state in numpy, vectorised over the vehicles, and the cells
    that hinge on rounding: (grid f64 [E, A, V, L, T], edge bool [E, A, V, L, T], candidates, smallest |q - rint(q)| seen).

    A candidate is one (other vehicle, ego speed, collision point): its time to collision q = ttc / tq (in cells) marks cell
    floor(q) and cell ceil(q) of the other vehicle's lane with the point's cost where they lie in [0, T).  ``edge`` marks the cells
    next to a candidate whose q lies within KNIFE of an integer, or whose closing speed lies within KNIFE of zero (the sign
    utils.not_zero gives it then hangs on the last bit of sin / cos)."""
    E, N, A = cfg.num_envs, cfg.num_vehicles, cfg.num_agents
    V, L, T = cfg.num_target_speeds, cfg.lanes_count, params.time_steps
    tq = params.time_quantization
    ts = np.array(cfg.target_speeds[:V])
    grid = np.zeros((E, A, V, L, T))
    edge = np.zeros((E, A, V, L, T), bool)
    closest, count = np.inf, 0
    shifts, costs = np.array([0.0, -MARGIN, MARGIN]), np.array([1.0, 0.5, 0.5])
    for e in range(E):
        for a in range(A):
            me = cfg.agent_index[a]
            others = np.flatnonzero((np.arange(N) != me) & ((st["flags"][e] & _abi.F_ABSENT) == 0))
            x, hd, sp, ln = (st[k][e][others] for k in ("x", "heading", "speed", "lane"))
            along = np.cos(hd) * np.cos(st["heading"][e, me]) + np.sin(hd) * np.sin(st["heading"][e, me])
            closing = ts[:, None] - (sp * along)[None, :]                                    # [V, n]
            near_zero = np.abs(closing) < KNIFE
            denom = np.where(np.abs(closing) > 1e-2, closing, np.where(closing >= 0, 1e-2, -1e-2))
            distance = (x - st["x"][e, me])[None, :, None] + shifts[None, None, :]           # [1, n, 3]
            ttc = distance / denom[:, :, None]                                              # [V, n, 3]
            q = ttc / tq
            differ = (ts[:, None] != sp[None, :])[:, :, None] & np.ones_like(q, bool)  # `ego_speed == other.speed`: skipped
            live = differ & ~(ttc < 0)
            count += int(live.sum())
            near = differ & (q > -KNIFE) & (q < T + 1)   # (a time within rounding of 0 may be skipped as negative, or kept)
            off = np.abs(q - np.rint(q))
            closest = min(closest, float(off[near].min(initial=np.inf)))
            for t in (np.floor(q), np.ceil(q)):   # both quantisations
                hit = live & (t >= 0) & (t < T)
                vi, oi, mi = np.nonzero(hit)
                np.maximum.at(grid[e, a], (vi, ln[oi], t[hit].astype(int)), costs[mi])
            for v, o, m in zip(*np.nonzero(differ & (near_zero[:, :, None] | (near & (off < KNIFE))))):
                if near_zero[v, o]:
                    edge[e, a, v, ln[o], :] = True
                else:
                    k = int(np.rint(q[v, o, m]))
                    edge[e, a, v, ln[o], max(k - 1, 0):max(min(k + 2, T), 0)] = True
    return grid, edge, count, closest


def fixed_point(transition, reward, terminal, gamma: float, sweeps: int):
    """``V <- max_a(reward + gamma * where(terminal, 0, V[transition]))`` from zeros, `sweeps` times, on the reference's recorded
    tables; one more sweep must change nothing.  Returns (V, Q)."""
    value = np.zeros(reward.shape[0])
    for _ in range(sweeps):
        q = reward + gamma * np.where(terminal[:, None], 0, value[transition])
        value = q.max(axis=1)
    q1 = reward + gamma * np.where(terminal[:, None], 0, value[transition])
    assert np.array_equal(q1, q) and np.array_equal(q1.max(axis=1), value), "the iteration has not reached its fixed point"
    return value, q


def highway_config(fast=True, **over) -> dict:
    d = _abi.highway_fast_default_config() if fast else _abi.highway_default_config()
    d.update(over)
    return d
