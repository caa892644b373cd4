#!/usr/bin/env python3
"""What a cross-entropy-method plan costs and what it buys at one shape (default: 256 x highway-fast-v0 x 51 vehicles, population 64,
horizon 8, 3 iterations):

 (a) plan_cem per call on the device (one hwy_cem_plan_device call between two events), and its stages: the fork of the parent into
     the work engine, the K (act, step) launch pairs and the fold, each timed on its own as the SAME call the planner makes; what
     remains of the plan after I x (fork + rollout + score), divided by the I (sample, refit) launch pairs, is reported as a residual
     (each stage sample carries the gap between two launches, so the residual bounds the two CEM kernels from below only);
 (b) the closed-loop mean return of `--envs` full episodes driven by plan_cem, by the zero action and by plan_opd on the matching
     3 x 3 DiscreteAction table (same seeds, same config).

    python tools/cem_bench.py [--envs 256] [--vehicles 50] [--population 64] [--elites 8] [--iterations 3] [--horizon 8] [--gamma 0.9]
                              [--repeats 20] [--warmup 5] [--no-episodes] [--out FILE.json]

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
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--vehicles", type=int, default=50)
    ap.add_argument("--population", type=int, default=64)
    ap.add_argument("--elites", type=int, default=8)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--gamma", type=float, default=0.9)
    ap.add_argument("--opd-budget", type=int, default=45)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-episodes", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    from highwayenv_amd import _abi, build
    from highwayenv_amd.vector import HighwayVectorEnv

    E, B, K, I = a.envs, a.population, a.horizon, a.iterations
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    config = {"vehicles_count": a.vehicles, "action": {"type": "DiscreteAction", "steering_range": [-0.1, 0.1], "actions_per_axis": 3}}
    kw = dict(population=B, elites=a.elites, iterations=I, horizon=K, gamma=a.gamma)

    def make(continuous=True):
        return HighwayVectorEnv("highway-fast-v0", E, config=config, output="torch", autoreset_mode="Disabled", stream=stream,
                                continuous=continuous)

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
            venv.step(torch.zeros((E, 2), dtype=torch.float32, device=dev))
    env = venv.env
    cp, cem, work = env._cem_setup(B, a.elites, I, K, a.gamma, 0.5, 0.05, 1.0, 0)
    result = {"what": "tools/cem_bench.py", "envs": E, "vehicles": env._hcfg.num_vehicles, "population": B, "elites": a.elites,
              "iterations": I, "horizon": K, "gamma": a.gamma, "work_envs": E * B, "kernel_source_hash": build.kernel_source_hash(),
              "device": torch.cuda.get_device_name(0)}

    # ---- (a) the plan, and its stages on their own ---------------------------------------------------------------------------------
    with torch.cuda.stream(stream):
        _, details = venv.plan_cem(seed=0, return_details=True, **kw)
    stream.synchronize()
    result["best_return_mean"] = float(details["best_return"].mean())
    (plan_ms,), (plan_s,) = timed([lambda: venv.plan_cem(seed=0, **kw)], a.repeats, a.warmup)
    n = E * B
    acts = (torch.rand((K, n, 1, 2), device=dev, dtype=torch.float32) * 2 - 1).contiguous()
    obs = torch.empty((K, n, 1, *_abi.obs_shape(env._hcfg)), dtype=torch.float32, device=dev)
    rew = torch.empty((K, n, 1), dtype=torch.float64, device=dev)
    term, trunc = torch.empty((K, n), dtype=torch.uint8, device=dev), torch.empty((K, n), dtype=torch.uint8, device=dev)
    ret = torch.empty((E, B, 1), dtype=torch.float64, device=dev)
    stream.synchronize()
    w = work._engine
    stages = [lambda: w.fork_device(env._engine, B),
              lambda: w.rollout_continuous_device(cp, K, acts.data_ptr(), obs.data_ptr(), rew.data_ptr(), term.data_ptr(), trunc.data_ptr()),
              lambda: w.score_device(K, B, a.gamma, 0, rew.data_ptr(), term.data_ptr(), trunc.data_ptr(), ret.data_ptr())]
    (fork_ms, roll_ms, score_ms), (fork_s, roll_s, score_s) = timed(stages, a.repeats, a.warmup)
    result["plan_cem"] = {"total_ms": plan_ms, "fork_ms": fork_ms, "rollout_ms": roll_ms, "score_ms": score_ms,
                          "residual_ms_per_sample_refit_pair": (plan_ms - I * (fork_ms + roll_ms + score_ms)) / I,
                          "total_ms_samples": plan_s, "fork_ms_samples": fork_s, "rollout_ms_samples": roll_s, "score_ms_samples": score_s}
    venv.close()

    # ---- (b) what the planner buys: mean return of E full episodes -------------------------------------------------------------------
    if not a.no_episodes:
        zero = torch.zeros((E, 2), dtype=torch.float32, device=dev)
        policies = {"plan_cem": (True, lambda v: v.plan_cem(**kw)), "zero_action": (True, lambda v: zero),
                    "plan_opd_3x3": (False, lambda v: v.plan_opd(a.opd_budget, 0.7))}
        result["episodes"] = {}
        for name, (continuous, policy) in policies.items():
            v = make(continuous)
            with torch.cuda.stream(stream):
                v.reset(seed=1000)
                total = torch.zeros(E, dtype=torch.float64, device=dev)
                length = torch.zeros(E, dtype=torch.int32, device=dev)
                alive = torch.ones(E, dtype=torch.bool, device=dev)
                crashed = torch.zeros(E, dtype=torch.bool, device=dev)
                for _ in range(int(v.env.config["duration"] * v.env.config["policy_frequency"])):
                    _, r, te, tr, info = v.step(policy(v))
                    total += torch.where(alive, r, torch.zeros_like(r))
                    length += alive.int()
                    crashed |= alive & info["crashed"]
                    alive = alive & ~(te | tr)
            stream.synchronize()
            result["episodes"][name] = {"mean_return": float(total.mean()), "mean_length": float(length.double().mean()),
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
