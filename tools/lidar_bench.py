#!/usr/bin/env python3
"""What the LidarObservation costs at one shape (default: 4096 x highway-fast-v0 x 50 vehicles, 4 lanes, 16 cells).

    python tools/lidar_bench.py --parent-tree DIR [--out profiles/lidar_bench.json]     the host-clock comparison
    python tools/lidar_bench.py --child lidar|kinematics [--root DIR]                  one measurement (one JSON line)
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/lidar_bench.py --child lidar --launches 200 --repeats 1
    python tools/lidar_bench.py --kernel-stats OUT [--merge profiles/lidar_bench.json]  the lidar kernel's average from that trace

Host clock: a child process steps one engine through `hwy_step_device` on device buffers (16 pre-staged random action planes,
auto-reset on) and times `--launches` steps between two stream synchronisations, `--repeats` times after a warm-up: microseconds
per policy step.  The comparison alternates children of THIS tree with the Lidar observation and of `--parent-tree` (a checkout
of the parent commit with its own library built) with its Kinematics observation, `--rounds` times in one session, and reports
every round so that the spread is visible next to the difference; a Kinematics child of this tree runs in every round too (the
step kernel is the parent's, byte for byte: tools/cmp_device_code.py).  The child uses nothing the parent commit lacks.

The kernel's own duration comes from a rocprofv3 kernel trace taken in a run of its own (tracing slows the host)."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a) -> None:
    root = os.path.abspath(a.root or HERE)
    sys.path.insert(0, root)
    import numpy as np
    import torch

    from highwayenv_amd import _abi, spawn
    from highwayenv_amd.engine import Engine

    E = a.envs
    d = _abi.highway_fast_default_config()
    d.update({"vehicles_count": a.vehicles, "lanes_count": a.lanes})
    if a.child == "lidar":
        d["observation"] = {"type": "LidarObservation", "cells": a.cells}
    cfg = _abi.make_config(d, E, fast=True)
    dev = torch.device("cuda", 0)
    eng = Engine(cfg, device=0)
    eng.set_state(spawn.spawn_reference_stream(cfg, np.arange(E), d["ego_spacing"], d["vehicles_density"]))
    eng.set_autoreset(True, base_seed=1, ego_spacing=d["ego_spacing"], vehicles_density=d["vehicles_density"])
    rng = np.random.default_rng(0)
    acts = [torch.from_numpy(rng.integers(0, 5, size=(E, 1)).astype(np.int32)).to(dev) for _ in range(16)]
    obs = torch.empty((E, 1, *_abi.obs_shape(cfg)), dtype=torch.float32, device=dev)
    rew = torch.empty((E, 1), dtype=torch.float64, device=dev)
    term, trunc = torch.empty(E, dtype=torch.uint8, device=dev), torch.empty(E, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def run(n):
        for k in range(n):
            eng.step_device(acts[k % 16].data_ptr(), obs.data_ptr(), rew.data_ptr(), term.data_ptr(), trunc.data_ptr())
        eng.sync()

    run(a.warmup)  # (also past the engine's own selection of the issue-priority turn: its first 85 .. 255 launches)
    us = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        run(a.launches)
        us.append((time.perf_counter() - t0) / a.launches * 1e6)
    checksum = float(obs.double().sum().item())
    eng.close()
    print(json.dumps({"obs": a.child, "root": "parent" if a.root else "tree", "envs": E, "vehicles": a.vehicles, "lanes": a.lanes,
                      "cells": a.cells if a.child == "lidar" else None, "launches": a.launches, "us_per_step": us,
                      "obs_checksum": checksum}))


def run_child(a, obs: str, root=None) -> dict:
    cmd = [sys.executable, os.path.abspath(__file__), "--child", obs, "--envs", str(a.envs), "--vehicles", str(a.vehicles), "--lanes",
           str(a.lanes), "--cells", str(a.cells), "--launches", str(a.launches), "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
    if root:
        cmd += ["--root", root]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=a.timeout).stdout
    return json.loads(out.strip().splitlines()[-1])


def compare(a) -> None:
    rounds = []
    for r in range(a.rounds):  # lidar / parent / this tree's Kinematics, alternated: drift of the machine hits them alike
        rounds.append({"lidar": run_child(a, "lidar")["us_per_step"],
                       "parent_kinematics": run_child(a, "kinematics", a.parent_tree)["us_per_step"],
                       "kinematics": run_child(a, "kinematics")["us_per_step"]})
        print(json.dumps(rounds[-1]), flush=True)

    def summary(key):
        v = sorted(x for r in rounds for x in r[key])
        return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "n": len(v)}

    res = {"shape": {"envs": a.envs, "vehicles": a.vehicles, "lanes": a.lanes, "cells": a.cells}, "launches_per_sample": a.launches,
           "host_clock_us_per_step": {k: summary(k) for k in ("lidar", "parent_kinematics", "kinematics")}, "rounds": rounds}
    h = res["host_clock_us_per_step"]
    res["lidar_minus_parent_us"] = h["lidar"]["median"] - h["parent_kinematics"]["median"]
    if a.out:
        prev = json.load(open(a.out)) if os.path.exists(a.out) else {}
        prev.update(res)
        with open(a.out, "w") as fh:
            json.dump(prev, fh, indent=1)
            fh.write("\n")
    print(json.dumps({k: res[k] for k in ("shape", "host_clock_us_per_step", "lidar_minus_parent_us")}))


def kernel_stats(a) -> None:
    """Average duration of every kernel of a rocprofv3 --kernel-trace --stats run (the *_kernel_stats.csv under the directory)."""
    files = glob.glob(os.path.join(a.kernel_stats, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {a.kernel_stats}")
    out = {}
    for row in csv.DictReader(open(sorted(files)[-1])):
        name = row["Name"].split("(")[0]
        out[name] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                     "max_us": float(row["MaxNs"]) / 1e3, "percent": float(row["Percentage"])}
    res = {"kernel_trace_us": out}
    if a.merge:
        prev = json.load(open(a.merge)) if os.path.exists(a.merge) else {}
        prev.update(res)
        with open(a.merge, "w") as fh:
            json.dump(prev, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["lidar", "kinematics"])
    ap.add_argument("--root")
    ap.add_argument("--parent-tree")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--merge")
    ap.add_argument("--out")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--vehicles", type=int, default=50)
    ap.add_argument("--lanes", type=int, default=4)
    ap.add_argument("--cells", type=int, default=16)
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=600)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240)
    a = ap.parse_args()
    if a.child:
        child(a)
    elif a.kernel_stats:
        kernel_stats(a)
    elif a.parent_tree:
        compare(a)
    else:
        ap.error("one of --child, --parent-tree, --kernel-stats")


if __name__ == "__main__":
    main()
