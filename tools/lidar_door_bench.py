#!/usr/bin/env python3
"""What a launch of the Lidar door's kernel (csrc/hwy_lidar_door.h) costs, next to the configured LidarObservation kernel
(csrc/hwy_lidar.h) on the same states.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/lidar_door_bench.py --child SHAPE [--launches 200]
    python tools/lidar_door_bench.py --kernel-stats OUT --shape SHAPE --merge profiles/lidar_door.json

Shapes (4096 environments each, the sizes a user runs):
  highway16    highway-fast-v0, 51 vehicles, 4 lanes, on a LIDAR-configured engine with 16 cells: after every policy step the
               configured kernel (`hwy_observe`) and the door with the same 16 cells trace the same state
  highway256   the same road on a Kinematics engine, the door with 256 cells (four cells per lane; no configured twin)
  merge_ma4    merge-generic, 43 slots, 4 agents (BASELINE config 5), the door with 16 cells

Kernel time is the kernel trace's (tracing slows the host, not the kernels); each shape is a process of its own so that the two
shapes that share an instantiation stay apart, and every shape is run several times: ``--kernel-stats`` appends one record per run,
so that the run-to-run spread stands next to the averages.  A run without a GPU fails: there is no fallback."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ("highway16", "highway256", "merge_ma4")


def child(a) -> None:
    sys.path.insert(0, HERE)
    import numpy as np

    from highwayenv_amd import _abi, merge
    from highwayenv_amd.engine import Engine

    E = a.envs
    if a.child == "merge_ma4":
        d = dict(merge.merge_generic_default_config(), lanes_count=4, vehicles_count=40, controlled_vehicles=4,
                 action={"type": "MultiAgentAction", "action_config": {"type": "DiscreteMetaAction"}},
                 observation={"type": "MultiAgentObservation", "observation_config": {"type": "Kinematics"}})
        cfg = _abi.make_config(d, E, scenario="merge-generic")
    else:
        d = dict(_abi.highway_fast_default_config(), vehicles_count=50, lanes_count=4)
        if a.child == "highway16":
            d["observation"] = {"type": "LidarObservation", "cells": 16}
        cfg = _abi.make_config(d, E, fast=True)
    params = _abi.lidar_door_params(256 if a.child == "highway256" else 16)
    eng = Engine(cfg, device=0)
    eng.reset(seeds=np.arange(E, dtype=np.uint64))
    eng.set_autoreset(True, base_seed=1)
    rng = np.random.default_rng(0)
    acts = [rng.integers(0, 5, size=(E, cfg.num_agents)).astype(np.int32) for _ in range(16)]
    checksum = 0.0
    for k in range(a.warmup + a.launches):
        eng.step(acts[k % 16])
        if a.child == "highway16":
            own = eng.observe()
        got = eng.lidar_observe(params)
        if a.child == "highway16":
            assert (own.view(np.uint32) == got.view(np.uint32)).all(), "the door and the configured kernel differ"
        checksum += float(got.sum(dtype=np.float64))
    eng.close()
    print(json.dumps({"shape": a.child, "envs": E, "slots": cfg.num_vehicles, "agents": cfg.num_agents, "cells": params.cells,
                      "launches": a.warmup + a.launches, "checksum": checksum}))


def kernel_stats(a) -> None:
    """The lidar kernels' rows of a rocprofv3 --kernel-trace --stats run (the *kernel_stats.csv under the directory), appended to
    the shape's list of runs in --merge."""
    files = glob.glob(os.path.join(a.kernel_stats, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {a.kernel_stats}")
    run = {}
    for row in csv.DictReader(open(sorted(files)[-1])):
        name = row["Name"].split("(")[0].removeprefix("void ")  # (the trace demangles with the return type of a template kernel)
        if "lidar" in name:
            run[name] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                         "max_us": float(row["MaxNs"]) / 1e3}
    if a.merge:
        prev = json.load(open(a.merge)) if os.path.exists(a.merge) else {}
        prev.setdefault(a.shape, []).append(run)
        with open(a.merge, "w") as fh:
            json.dump(prev, fh, indent=1)
            fh.write("\n")
    print(json.dumps({a.shape: run}))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=SHAPES)
    ap.add_argument("--kernel-stats")
    ap.add_argument("--shape", choices=SHAPES)
    ap.add_argument("--merge")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if a.child:
        child(a)
    elif a.kernel_stats and a.shape:
        kernel_stats(a)
    else:
        ap.error("--child SHAPE, or --kernel-stats DIR --shape SHAPE")


if __name__ == "__main__":
    main()
