#!/usr/bin/env python3
"""What an optimistic plan costs and what it buys at one shape (default: 4096 x highway-fast-v0 x 51 vehicles, budget 50, gamma 0.7):

 (a) plan_opd per call on the device (one hwy_opd_plan_device call between two events), and its stages: the gather tree -> work,
     the work engine's step and the scatter work -> tree, each timed on its own as the SAME call with index arrays of the same
     shape as the planner's (gather: every work environment from a tree slot; scatter: -1 everywhere but n slots per tree); what
     remains of the plan after X x (gather + step + scatter), divided by the X + 1 launches of the tree kernel, is reported as a
     residual (each stage sample carries the gap between two launches, so the residual bounds the tree kernel from below only);
 (b) plan_lookahead(2) and plan_lookahead(3) per call in the same run;
 (c) the mean return of `--envs` full episodes driven by plan_opd, by plan_lookahead(2, gamma) and by IDLE (same seeds).

    python tools/opd_bench.py [--envs 4096] [--vehicles 50] [--budget 50] [--gamma 0.7] [--repeats 20] [--warmup 5] [--no-episodes]
                              [--out FILE.json]

One process; every device sample is one call between two events recorded on the engine's stream, after `--warmup` calls; the
summary of each kind is the median of `--repeats` samples (the samples are reported too).  Prints one JSON line and, with --out,
writes it."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--vehicles", type=int, default=50)
    ap.add_argument("--budget", type=int, default=50)
    ap.add_argument("--gamma", type=float, default=0.7)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-episodes", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    from highwayenv_amd import _abi, build
    from highwayenv_amd.vector import HighwayVectorEnv

    E = a.envs
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    config = {"vehicles_count": a.vehicles}

    def make():
        return HighwayVectorEnv("highway-fast-v0", E, config=config, output="torch", autoreset_mode="Disabled", stream=stream)

    def timed(fns, repeats, warmup):
        """Median device ms of every stage of `fns` (run back to back on the stream), and the samples."""
        samples = [[] for _ in fns]
        for it in range(warmup + repeats):
            with torch.cuda.stream(stream):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)]
                ev[0].record(stream)
                for fn, e in zip(fns, ev[1:]):
                    fn()
                    e.record(stream)
            ev[-1].synchronize()
            if it >= warmup:
                for k in range(len(fns)):
                    samples[k].append(ev[k].elapsed_time(ev[k + 1]))
        return [float(np.median(s)) for s in samples], samples

    venv = make()
    with torch.cuda.stream(stream):
        venv.reset(seed=0)
        for _ in range(5):   # into the middle of the episodes
            venv.step(torch.randint(0, 5, (E,), dtype=torch.int32, device=dev))
    env = venv.env
    params, tree, work = env._opd_setup(a.budget, a.gamma)
    n, M, X = params.n_ids, params.nodes, params.budget // params.n_ids
    result = {"what": "tools/opd_bench.py", "envs": E, "vehicles": env._hcfg.num_vehicles, "budget": a.budget, "gamma": a.gamma,
              "n_ids": n, "nodes": M, "expansions": X, "tree_envs": E * M, "work_envs": E * n,
              "kernel_source_hash": build.kernel_source_hash(), "device": torch.cuda.get_device_name(0)}

    # ---- (a) the plan, and its stages on their own ---------------------------------------------------------------------------------
    with torch.cuda.stream(stream):
        action, details = venv.plan_opd(a.budget, a.gamma, return_details=True)
    stream.synchronize()
    result["expanded_mean"] = float(details["expanded"].double().mean())
    (plan_ms,), (plan_s,) = timed([lambda: venv.plan_opd(a.budget, a.gamma)], a.repeats, a.warmup)
    e_idx = torch.arange(E, device=dev, dtype=torch.int32)
    gather = (e_idx[:, None] * M + 1 + torch.arange(n, device=dev, dtype=torch.int32)[None, :]).reshape(-1).contiguous()   # existing slots
    scatter = torch.full((E, M), -1, dtype=torch.int32, device=dev)
    scatter[:, 1 + n:1 + 2 * n] = e_idx[:, None] * n + torch.arange(n, device=dev, dtype=torch.int32)[None, :]
    acts = (torch.arange(E * n, device=dev, dtype=torch.int32) % n).contiguous()
    obs = torch.empty((E * n, 1, *_abi.obs_shape(env._hcfg)), dtype=torch.float32, device=dev)
    rew = torch.empty((E * n, 1), dtype=torch.float64, device=dev)
    term, trunc = torch.empty(E * n, dtype=torch.uint8, device=dev), torch.empty(E * n, dtype=torch.uint8, device=dev)
    stream.synchronize()
    stages = [lambda: work._engine.fork_device(tree._engine, 1, gather.data_ptr()),
              lambda: work._engine.step_device(acts.data_ptr(), obs.data_ptr(), rew.data_ptr(), term.data_ptr(), trunc.data_ptr()),
              lambda: tree._engine.fork_device(work._engine, 1, scatter.data_ptr())]
    (gather_ms, step_ms, scatter_ms), (gather_s, step_s, scatter_s) = timed(stages, a.repeats, a.warmup)
    kernel_ms = (plan_ms - X * (gather_ms + step_ms + scatter_ms)) / (X + 1)
    result["plan_opd"] = {"total_ms": plan_ms, "gather_ms": gather_ms, "step_ms": step_ms, "scatter_ms": scatter_ms,
                          "residual_ms_per_tree_kernel_launch": kernel_ms, "total_ms_samples": plan_s, "gather_ms_samples": gather_s,
                          "step_ms_samples": step_s, "scatter_ms_samples": scatter_s}

    # ---- (b) the exhaustive lookahead in the same run ----------------------------------------------------------------------------------
    result["plan_lookahead"] = {}
    for depth in (2, 3):
        with torch.cuda.stream(stream):
            venv.plan_lookahead(depth, gamma=a.gamma)
        stream.synchronize()
        (ms,), (s,) = timed([lambda: venv.plan_lookahead(depth, gamma=a.gamma)], a.repeats, a.warmup)
        result["plan_lookahead"][f"depth{depth}"] = {"branch_envs": E * n ** depth, "total_ms": ms, "total_ms_samples": s}
        for key in [k for k in venv._dev if isinstance(k, tuple) and k[0] == "lookahead"]:   # give the branch engines back
            del venv._dev[key]
        for key in [k for k in env._forks if isinstance(k[0], int)]:
            env._forks.pop(key).close()
    venv.close()

    # ---- (c) what the planners buy: mean return of E full episodes ---------------------------------------------------------------------
    if not a.no_episodes:
        policies = {"plan_opd": lambda v: v.plan_opd(a.budget, a.gamma), "plan_lookahead2": lambda v: v.plan_lookahead(2, gamma=a.gamma),
                    "idle": lambda v: torch.ones(E, dtype=torch.int32, device=dev)}
        result["episodes"] = {}
        for name, policy in policies.items():
            v = make()
            with torch.cuda.stream(stream):
                v.reset(seed=1000)
                ret = torch.zeros(E, dtype=torch.float64, device=dev)
                length = torch.zeros(E, dtype=torch.int32, device=dev)
                alive = torch.ones(E, dtype=torch.bool, device=dev)
                crashed = torch.zeros(E, dtype=torch.bool, device=dev)
                for _ in range(int(v.env.config["duration"] * v.env.config["policy_frequency"])):
                    _, r, te, tr, info = v.step(policy(v))
                    ret += torch.where(alive, r, torch.zeros_like(r))
                    length += alive.int()
                    crashed |= alive & info["crashed"]
                    alive = alive & ~(te | tr)
            stream.synchronize()
            result["episodes"][name] = {"mean_return": float(ret.mean()), "mean_length": float(length.double().mean()),
                                        "crashed_fraction": float(crashed.double().mean()), "still_running": int(alive.sum())}
            v.close()
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
