#!/usr/bin/env python3
"""What the time-to-collision grid and the finite-MDP planner cost at one shape (default: 4096 x highway-fast-v0 x 51 vehicles,
4 lanes, grid 3 x 4 x 10): device time per launch of the grid alone (hwy_ttc_grid_device), of grid + plan (hwy_mdp_plan_device)
and, beside them, of the step kernel of the same build on the same device and state (hwy_step_device).

    python tools/ttc_bench.py [--envs 4096] [--vehicles 50] [--lanes 4] [--launches 300] [--rounds 3] [--out profiles/ttc_bench.json]

Each sample is `--launches` back-to-back launches on the engine's stream between two events recorded on that stream (the elapsed
time divided by the number of launches: kernel time plus the gap between consecutive dispatches), after a warm-up that also steps the
engine into the middle of its episodes (and past its own selection of the issue-priority turn).  The three kinds alternate in
`--rounds` rounds, so that clock drift hits them alike; every round is reported, the summary is the median.  The step kernel's own
dispatch time (hwy_profile_*) is reported too.  Prints one JSON line and, with --out, writes it."""
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
    ap.add_argument("--lanes", type=int, default=4)
    ap.add_argument("--policy-frequency", type=int, default=1)
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--gamma", type=float, default=0.9)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    from highwayenv_amd import _abi, build, spawn
    from highwayenv_amd.engine import Engine

    E = a.envs
    d = _abi.highway_fast_default_config()
    d.update({"vehicles_count": a.vehicles, "lanes_count": a.lanes, "policy_frequency": a.policy_frequency})
    cfg = _abi.make_config(d, E, fast=True)
    params = _abi.ttc_params(d, gamma=a.gamma)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    eng = Engine(cfg, device=0, stream=stream.cuda_stream)
    eng.set_state(spawn.spawn_reference_stream(cfg, np.arange(E), d["ego_spacing"], d["vehicles_density"]))
    eng.set_autoreset(True, base_seed=1, ego_spacing=d["ego_spacing"], vehicles_density=d["vehicles_density"])
    rng = np.random.default_rng(0)
    acts = [torch.from_numpy(rng.integers(0, 5, size=(E, 1)).astype(np.int32)).to(dev) for _ in range(16)]
    out = (torch.empty((E, 1, *_abi.obs_shape(cfg)), dtype=torch.float32, device=dev), torch.empty((E, 1), dtype=torch.float64, device=dev),
           torch.empty(E, dtype=torch.uint8, device=dev), torch.empty(E, dtype=torch.uint8, device=dev))
    shape = eng.ttc_shape(params)
    grid = torch.empty((E, 1, *shape), dtype=torch.float32, device=dev)
    plan = torch.empty((E, 1), dtype=torch.int32, device=dev)
    q = torch.empty((E, 1, 5), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    k = [0]

    def step():
        eng.step_device(acts[k[0] % 16].data_ptr(), *(t.data_ptr() for t in out))
        k[0] += 1

    kinds = {"step": step,
             "ttc_grid": lambda: eng.ttc_grid_device(params, grid.data_ptr()),
             "grid_and_plan": lambda: eng.mdp_plan_device(params, plan.data_ptr(), q.data_ptr(), grid.data_ptr()),
             "plan_action_only": lambda: eng.mdp_plan_device(params, plan.data_ptr())}

    def timed(fn, n):
        with torch.cuda.stream(stream):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            for _ in range(n):
                fn()
            t1.record(stream)
        t1.synchronize()
        return 1000.0 * t0.elapsed_time(t1) / n

    timed(step, a.warmup)
    for name, fn in kinds.items():
        timed(fn, 50)
    us = {name: [] for name in kinds}
    step_dispatch = []
    for _ in range(a.rounds):
        for name, fn in kinds.items():
            us[name].append(timed(fn, a.launches))
        eng.profile_enable(1)  # (a run of its own: the timed launch records two more events per dispatch)
        timed(step, a.launches)
        ms, n = eng.profile_read()
        eng.profile_enable(0)
        step_dispatch.append(1000.0 * ms / n)
    marked = float((grid > 0).float().mean().item())
    actions = np.bincount(plan.cpu().numpy().ravel(), minlength=5).tolist()
    res = {"shape": f"{E} x highway-fast-v0 x {a.vehicles + 1} vehicles, {a.lanes} lanes, grid {shape[0]} x {shape[1]} x {shape[2]}",
           "launches_per_round": a.launches, "rounds": a.rounds,
           "us_per_launch": {n: round(float(np.median(v)), 2) for n, v in us.items()},
           "us_per_round": {n: [round(x, 2) for x in v] for n, v in us.items()},
           "step_kernel_dispatch_us": round(float(np.median(step_dispatch)), 2),
           "grid_over_step": round(float(np.median(us["ttc_grid"]) / np.median(us["step"])), 3),
           "grid_and_plan_over_step": round(float(np.median(us["grid_and_plan"]) / np.median(us["step"])), 3),
           "f64_divisions_per_row": 6 * a.vehicles * shape[0],
           "marked_cells": round(marked, 4), "planned_actions_histogram": actions,
           "kernel_source_hash": build.kernel_source_hash(), "device": torch.cuda.get_device_name(0)}
    eng.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
