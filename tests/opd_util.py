"""Shared helpers of the optimistic-planner tests (``plan_opd``, csrc/hwy_opd.h): the backends (``emu`` = tests/emu/emu.py on
the CPU, ``hip`` = the engine on the MI355X), the environment classes on either, and the YARDSTICK: ``restate_opd``, a plain
Python / NumPy restatement of the rules of DESIGN.md ("OPD on the device").  It keeps every node's state on the host (get_state /
set_state, Linear behaviour and stored controls included), steps the children with the ordinary ``step`` of a scratch engine of the
same backend (auto-reset off), and computes the bounds in f64 with the same statements as the kernel, one product or sum each.
Comparisons with it are exact: action, sequence, expanded, and the bits of value / upper."""
from __future__ import annotations

import numpy as np

from highwayenv_amd import _abi
from tests.backends import BACKENDS, make_engine  # noqa: F401  (re-exported)
from tests.lookahead_util import assert_bits, env_class, with_envs  # noqa: F401  (re-exported)

STATE_KEYS = _abi.STATE_F64 + _abi.STATE_I32 + ["time"]


def fast_config(vehicles: int = 8, **over) -> dict:
    """highway-fast-v0 (its frequencies, 3 lanes) with ``vehicles`` traffic vehicles."""
    d = _abi.highway_fast_default_config()
    d.update({"vehicles_count": vehicles, **over})
    return d


def make_env(backend: str, config: dict, num_envs: int, seed: int, warm=()):
    """A reset environment; ``warm``: actions (one id for all environments per entry) stepped before the plan."""
    env = env_class(backend)(config, num_envs=num_envs)
    env.reset(seed=seed)
    for a in warm:
        env.step(np.full(num_envs, a, np.int32))
    return env


class HostStates:
    """The states of a set of environments on the host: the planes of get_state, the Linear family's behaviour parameters and the
    stored controls of a direct-control ego, row by row."""

    def __init__(self, cfg):
        self.linear = cfg.traffic_model == _abi.TRAFFIC_LINEAR
        self.direct = cfg.ego_control == _abi.EGO_DIRECT

    def read(self, eng) -> list:
        st = eng.get_state()
        beh = eng.get_behavior() if self.linear else None
        ctl = eng.get_controls() if self.direct else None
        return [{"st": {k: np.array(st[k][e]) for k in STATE_KEYS}, "beh": None if beh is None else beh[e].copy(),
                 "ctl": None if ctl is None else (ctl[0][e].copy(), ctl[1][e].copy())} for e in range(eng.E)]

    def write(self, eng, rows: list):
        eng.set_state({k: np.stack([r["st"][k] for r in rows]) for k in STATE_KEYS})
        if self.linear:
            eng.set_behavior(np.stack([r["beh"] for r in rows]))
        if self.direct:
            eng.set_controls(np.stack([r["ctl"][0] for r in rows]), np.stack([r["ctl"][1] for r in rows]))


def _backup(nodes):
    """Value lower / upper of every expanded node = the maximum over its children, the expanded nodes in reverse creation order."""
    for node in reversed(nodes):
        if node["children"] is not None:
            node["vlo"] = max(nodes[c]["vlo"] for c in node["children"])
            node["vup"] = max(nodes[c]["vup"] for c in node["children"])


def restate_opd(backend: str, env, budget: int, gamma: float) -> dict:
    """The plan of every environment of ``env`` by the rules, and what the tests want to know about the trees: ``action``,
    ``value``, ``upper``, ``sequence``, ``expanded`` as ``plan_opd`` returns them, and per environment ``trees`` (the node lists),
    ``tie`` (a selection met two leaves of equal value upper) and ``solved``."""
    cfg = env._hcfg
    E, n = env.num_envs, _abi.num_actions(cfg)
    X = int(budget) // n
    gamma = np.float64(gamma)
    bound = np.float64(1.0) / (np.float64(1.0) - gamma)
    scratch = make_engine(backend, with_envs(cfg, E * n))
    scratch.set_autoreset(False)
    host = HostStates(cfg)
    roots = host.read(env._engine)
    trees = [[{"state": roots[e], "ret": np.float64(0.0), "vlo": np.float64(0.0), "vup": bound, "disc": np.float64(1.0),
               "done": False, "children": None, "parent": -1, "act": -1}] for e in range(E)]
    expanded, tie, held = np.zeros(E, np.int32), np.zeros(E, bool), [None] * E
    for x in range(X):
        picks = []
        for e in range(E):
            nodes = trees[e]
            _backup(nodes)
            leaves = [i for i, nd in enumerate(nodes) if nd["children"] is None]
            top = max(nodes[i]["vup"] for i in leaves)
            holders = [i for i in leaves if nodes[i]["vup"] == top]
            tie[e] |= len(holders) > 1
            leaf = holders[0]                                   # ties: the lowest node index
            picks.append(None if nodes[leaf]["done"] else leaf)  # a done leaf: the tree is solved, the expansion void
        if all(p is None for p in picks):
            break
        # one step of the scratch engine: environment e * n + a is the picked leaf of e under action a (a void tree: what it held)
        for e in range(E):
            if picks[e] is not None:
                held[e] = trees[e][picks[e]]["state"]
            elif held[e] is None:
                held[e] = roots[e]
        host.write(scratch, [held[e] for e in range(E) for _ in range(n)])
        _, reward, term, trunc, _ = scratch.step(np.tile(np.arange(n, dtype=np.int32), E).reshape(E * n, 1))
        after = host.read(scratch)
        for e in range(E):
            p = picks[e]
            if p is None:
                continue
            nodes, parent = trees[e], trees[e][p]
            parent["children"] = []
            for a in range(n):
                j = e * n + a
                t = parent["disc"] * np.float64(reward[j, 0])
                lower = parent["ret"] + t
                disc = parent["disc"] * gamma
                done = bool(term[j]) or bool(trunc[j])
                if done:
                    upper = lower
                else:
                    u = disc * bound
                    upper = lower + u
                parent["children"].append(len(nodes))
                nodes.append({"state": after[j], "ret": lower, "vlo": lower, "vup": upper, "disc": disc, "done": done,
                              "children": None, "parent": p, "act": a})
            expanded[e] += 1
    out = {"action": np.zeros(E, np.int32), "value": np.zeros(E), "upper": np.zeros(E), "sequence": np.full((E, X), -1, np.int32),
           "expanded": expanded, "trees": trees, "tie": tie, "solved": expanded < X}
    for e in range(E):
        nodes = trees[e]
        _backup(nodes)
        out["value"][e], out["upper"][e] = nodes[0]["vlo"], nodes[0]["vup"]
        node, d = nodes[0], 0
        while node["children"] is not None:
            vals = [nodes[c]["vlo"] for c in node["children"]]
            a = int(np.argmax(vals))                            # ties: the lowest id
            out["sequence"][e, d] = a
            node, d = nodes[node["children"][a]], d + 1
        out["action"][e] = out["sequence"][e, 0]
    scratch.close()
    return out


def assert_plan_equals(got_action, got: dict, want: dict, what=""):
    np.testing.assert_array_equal(got_action, want["action"], err_msg=f"{what}: action")
    np.testing.assert_array_equal(got["expanded"], want["expanded"], err_msg=f"{what}: expanded")
    np.testing.assert_array_equal(got["sequence"], want["sequence"], err_msg=f"{what}: sequence")
    assert_bits(np.asarray(got["value"], np.float64), want["value"], f"{what}: value")
    assert_bits(np.asarray(got["upper"], np.float64), want["upper"], f"{what}: upper")


def depth_min(tree: list) -> int:
    """The depth of the shallowest leaf of a restated tree."""
    def depth(i):
        d = 0
        while tree[i]["parent"] >= 0:
            i, d = tree[i]["parent"], d + 1
        return d
    return min(depth(i) for i, nd in enumerate(tree) if nd["children"] is None)
