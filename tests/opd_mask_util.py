"""The YARDSTICK of the masked optimistic planner (``plan_opd(masked=True)``, csrc/hwy_opd.h with HWY_OPD_MASKED): ``restate_masked_opd``,
tests/opd_util.py's plain Python restatement with the one rule added -- a node's unavailable actions (the action mask of its state)
get no child -- and the helpers of its tests.  The budget still buys ``budget // n_ids`` expansions; backup, selection (ties: the
node created first), the root's argmax and the greedy sequence (ties: the lowest action id) run over the created children."""
from __future__ import annotations

import numpy as np

from highwayenv_amd import _abi
from tests import opd_util
from tests.lookahead_util import with_envs
from tests.opd_util import BACKENDS, HostStates, assert_plan_equals, env_class, fast_config, make_engine  # noqa: F401  (re-exported)


def make_env(backend: str, config: dict, num_envs: int, seed: int, warm=()):
    env = env_class(backend)(config, num_envs=num_envs)
    env.reset(seed=seed)
    for a in warm:
        env.step(np.broadcast_to(np.asarray(a, np.int32), (num_envs,)))
    return env


def restate_masked_opd(backend: str, env, budget: int, gamma: float) -> dict:
    """opd_util.restate_opd with masks: ``action``, ``value``, ``upper``, ``sequence``, ``expanded`` as ``plan_opd(masked=True)``
    returns them, ``trees`` (node lists; a node holds the ``mask`` of its state once it is expanded) and ``masked_out`` (children
    not created, per environment)."""
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
    expanded, masked_out, held = np.zeros(E, np.int32), np.zeros(E, np.int32), [None] * E
    for x in range(X):
        picks = []
        for e in range(E):
            nodes = trees[e]
            opd_util._backup(nodes)
            leaves = [i for i, nd in enumerate(nodes) if nd["children"] is None]
            top = max(nodes[i]["vup"] for i in leaves)
            leaf = [i for i in leaves if nodes[i]["vup"] == top][0]   # ties: the node created first (the lowest slot)
            picks.append(None if nodes[leaf]["done"] else leaf)
        if all(p is None for p in picks):
            break
        for e in range(E):
            if picks[e] is not None:
                held[e] = trees[e][picks[e]]["state"]
            elif held[e] is None:
                held[e] = roots[e]
        host.write(scratch, [held[e] for e in range(E) for _ in range(n)])
        mask = scratch.action_mask()[:, 0]                            # rows e * n .. e * n + n - 1: n copies of the leaf of e
        _, reward, term, trunc, _ = scratch.step(np.tile(np.arange(n, dtype=np.int32), E).reshape(E * n, 1))
        after = host.read(scratch)
        for e in range(E):
            p = picks[e]
            if p is None:
                continue
            nodes, parent = trees[e], trees[e][p]
            parent["children"], parent["mask"] = [], mask[e * n].copy()
            assert mask[e * n, 1]                                     # IDLE: an expanded node always has a child
            for a in range(n):
                if not mask[e * n, a]:
                    masked_out[e] += 1
                    continue
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
           "expanded": expanded, "trees": trees, "masked_out": masked_out}
    for e in range(E):
        nodes = trees[e]
        opd_util._backup(nodes)
        out["value"][e], out["upper"][e] = nodes[0]["vlo"], nodes[0]["vup"]
        node, d = nodes[0], 0
        while node["children"] is not None:
            vals = [nodes[c]["vlo"] for c in node["children"]]
            child = nodes[node["children"][int(np.argmax(vals))]]     # ties: the lowest id among the created children
            out["sequence"][e, d] = child["act"]
            node, d = child, d + 1
        out["action"][e] = out["sequence"][e, 0]
    scratch.close()
    return out


def replay_is_available(backend: str, env, sequence) -> int:
    """Replays ``sequence`` [E, X] (-1 padded) on a fork of ``env``: every action must be available in the state it is applied to.
    Returns the number of actions checked."""
    child = env.fork(1)
    E, checked = env.num_envs, 0
    for d in range(sequence.shape[1]):
        live = sequence[:, d] >= 0
        if not live.any():
            break
        mask = child.get_available_actions()
        assert mask[np.flatnonzero(live), sequence[live, d]].all(), f"step {d}: an unavailable action in the sequence"
        checked += int(live.sum())
        child.step(np.where(live, sequence[:, d], 1).astype(np.int32))
    return checked
