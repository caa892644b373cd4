#!/usr/bin/env python3
"""IDM against LinearVehicle-family traffic at one shape (default: 4096 x highway-fast-v0 x 50 vehicles, 4 lanes): the kernel's
own duration per policy step (hwy_profile_*: the dispatch's begin / end timestamps, HIP events) over >= 300 launches after a
warm-up, the two models alternated in rounds so that clock drift hits both alike.  Prints one JSON line.

    python tools/traffic_bench.py [--envs 4096] [--vehicles 50] [--lanes 4] [--launches 300] [--rounds 3]

Both models run on the one-wavefront kernel (hwy_wave.h) for N <= 64; "idm_workgroup" / "linear_workgroup" time the workgroup
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
    variants = {"idm": ("IDMVehicle", 0), "linear": ("LinearVehicle", 0), "idm_workgroup": ("IDMVehicle", 1),
                "linear_workgroup": ("LinearVehicle", 1)}
    dev = torch.device("cuda", 0)
    engines, bufs = {}, {}
    for name, (cls, block) in variants.items():
        d = _abi.highway_fast_default_config()
        d.update({"vehicles_count": a.vehicles, "lanes_count": a.lanes, "other_vehicles_type": "highway_env.vehicle.behavior." + cls})
        cfg = _abi.make_config(d, E, fast=True, tuning={"block_kernel": block})
        eng = Engine(cfg, device=0)
        st = spawn.spawn_reference_stream(cfg, np.arange(E), d["ego_spacing"], d["vehicles_density"])
        eng.set_state(st)
        if "behavior" in st:
            eng.set_behavior(st["behavior"])
        eng.set_autoreset(True, base_seed=1, ego_spacing=d["ego_spacing"], vehicles_density=d["vehicles_density"])
        acts = torch.from_numpy(np.random.default_rng(0).integers(0, 5, size=(E, 1)).astype(np.int32)).to(dev)
        out = (torch.empty((E, 1, *_abi.obs_shape(cfg)), dtype=torch.float32, device=dev),
               torch.empty((E, 1), dtype=torch.float64, device=dev), torch.empty(E, dtype=torch.uint8, device=dev),
               torch.empty(E, dtype=torch.uint8, device=dev))
        engines[name], bufs[name] = eng, (acts, out)

    def run(name, n):
        eng, (acts, out) = engines[name], bufs[name]
        for _ in range(n):
            eng.step_device(acts.data_ptr(), *(t.data_ptr() for t in out))

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
           "us_per_round": {k: [round(x, 2) for x in v] for k, v in us.items()}}
    res["linear_over_idm"] = round(res["us_per_step"]["linear"] / res["us_per_step"]["idm"], 3)
    res["linear_workgroup_over_idm_workgroup"] = round(res["us_per_step"]["linear_workgroup"] / res["us_per_step"]["idm_workgroup"], 3)
    for eng in engines.values():
        eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
