#!/usr/bin/env python3
"""Meta-action (DiscreteMetaAction) against direct (DiscreteAction) ego control at one shape (default: 4096 x highway-fast-v0 x
50 vehicles, 4 lanes): the kernel's own duration per policy step (hwy_profile_*: the dispatch's begin / end timestamps, HIP
events) over 3 x 300 launches after a warm-up, the variants alternated in rounds so that clock drift hits them alike.  Both run in
the SAME build on the same device; the meta-action kernel is the yardstick.  Prints one JSON line.

    python tools/control_bench.py [--envs 4096] [--vehicles 50] [--lanes 4] [--launches 300] [--rounds 3]

Every launch takes the next of 16 pre-staged random action planes (ids uniform over each variant's table; the direct variant's
steering range is +-0.05 rad so that its egos meander inside the traffic instead of leaving the road), auto-reset on.  Both
variants run on the one-wavefront kernel (hwy_wave.h) for N <= 64; "meta_workgroup" / "direct_workgroup" time the workgroup
kernel (hwy_device.h, tune_block_kernel = 1), which N > 64 runs."""
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
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import torch

    from highwayenv_amd import _abi, spawn
    from highwayenv_amd.engine import Engine

    E = a.envs
    meta, direct = {"type": "DiscreteMetaAction"}, {"type": "DiscreteAction", "steering_range": [-0.05, 0.05]}
    variants = {"meta": (meta, 0), "direct": (direct, 0), "meta_workgroup": (meta, 1), "direct_workgroup": (direct, 1)}
    dev = torch.device("cuda", 0)
    engines, bufs = {}, {}
    for name, (action, block) in variants.items():
        d = _abi.highway_fast_default_config()
        d.update({"vehicles_count": a.vehicles, "lanes_count": a.lanes, "action": action})
        cfg = _abi.make_config(d, E, fast=True, tuning={"block_kernel": block})
        eng = Engine(cfg, device=0)
        eng.set_state(spawn.spawn_reference_stream(cfg, np.arange(E), d["ego_spacing"], d["vehicles_density"]))
        eng.set_autoreset(True, base_seed=1, ego_spacing=d["ego_spacing"], vehicles_density=d["vehicles_density"])
        rng = np.random.default_rng(0)
        acts = [torch.from_numpy(rng.integers(0, _abi.num_actions(cfg), size=(E, 1)).astype(np.int32)).to(dev) for _ in range(16)]
        out = (torch.empty((E, 1, *_abi.obs_shape(cfg)), dtype=torch.float32, device=dev),
               torch.empty((E, 1), dtype=torch.float64, device=dev), torch.empty(E, dtype=torch.uint8, device=dev),
               torch.empty(E, dtype=torch.uint8, device=dev))
        engines[name], bufs[name] = eng, (acts, out, [0])

    def run(name, n):
        eng, (acts, out, k) = engines[name], bufs[name]
        for _ in range(n):
            eng.step_device(acts[k[0] % 16].data_ptr(), *(t.data_ptr() for t in out))
            k[0] += 1

    for name in variants:  # warm-up (and the engine's own issue-priority turn selection)
        run(name, a.warmup)
        engines[name].sync()
    us = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name in variants:
            eng = engines[name]
            eng.profile_enable(1)
            run(name, a.launches)
            ms, n = eng.profile_read()
            eng.profile_enable(0)
            us[name].append(1000.0 * ms / n)
    res = {"shape": f"{E} x highway-fast-v0 x {a.vehicles + 1} vehicles, {a.lanes} lanes", "launches_per_round": a.launches,
           "rounds": a.rounds, "us_per_step": {k: round(float(np.median(v)), 2) for k, v in us.items()},
           "us_per_round": {k: [round(x, 2) for x in v] for k, v in us.items()},
           "spread_us": {k: round(max(v) - min(v), 2) for k, v in us.items()},
           "prio_turn": {k: engines[k].prio_turn()[0] for k in variants}}
    res["direct_over_meta"] = round(res["us_per_step"]["direct"] / res["us_per_step"]["meta"], 3)
    res["direct_workgroup_over_meta_workgroup"] = round(res["us_per_step"]["direct_workgroup"] / res["us_per_step"]["meta_workgroup"], 3)
    for eng in engines.values():
        eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
