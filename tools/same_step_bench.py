#!/usr/bin/env python3
"""What SameStep on the device costs: per-call device time of hwy_step_device under the next-step auto-reset against
hwy_step_same_step_device, from the same build, on the same device, in steady state with the natural rate of episode ends.

    python tools/same_step_bench.py [--envs 4096] [--launches 310] [--rounds 5] [--configs fast,v0] [--skip-frontends] [--out FILE]

Two shapes: the headline (highway-fast-v0 x 4096 x 50 vehicles, 4 lanes, duration 30) and highway-v0 x 4096 (50 vehicles, 4 lanes,
duration 40).  Per shape two engines on one stream, reset alike on the device; during the warm-up (one episode length) a slice of
the environments is reset again after every call, so that the time limits are spread evenly over the calls instead of all falling
into one -- afterwards about one environment in `duration` ends per call, plus the crashes.  Each sample is `--launches`
back-to-back calls between two events recorded on the engine's stream (elapsed time / calls: kernel time plus the gaps between the
dispatches of a call); the kinds alternate in `--rounds` rounds, every round is reported, the summary is the median and the spread
max - min over the rounds.  Kinds:
  next_step         hwy_step_device, auto-reset on: an environment that ended is re-spawned INSTEAD of stepped by the next call
  same_step         hwy_step_same_step_device with both final info planes: step + stash + re-spawn
  same_step_masks   the same with both action-mask planes: + two launches of the mask kernel
  step_kernel_*     the step kernel's own dispatch time in either mode (hwy_profile_enable: begin / end timestamps of the dispatch)
same_step - step_kernel_same_step is what the two extra launches (stash, re-spawn) and their dispatch gaps add to a call.
us per USEFUL env-step: under next-step the re-spawn rows (reward 0, action ignored) are not useful steps -- elapsed time over
(calls x envs - re-spawn rows); under same-step every row is one.
Then the front ends, wall time per step() ending in a device synchronise: HighwayVectorEnv(output="torch") with NextStep and with
SameStep, and the numpy SameStep front end (flags to the host, masked hwy_reset, object arrays) that the device path replaces.
Prints one JSON line and, with --out, writes it."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"fast": ("highway-fast-v0", True, {"vehicles_count": 50, "lanes_count": 4}),
          "v0": ("highway-v0", False, {"vehicles_count": 50, "lanes_count": 4})}


def device_section(a, torch, name) -> dict:
    from highwayenv_amd import _abi
    from highwayenv_amd.engine import Engine
    env_id, fast, over = SHAPES[name]
    d = _abi.highway_fast_default_config() if fast else _abi.highway_default_config()
    d.update(over)
    E = a.envs
    cfg = _abi.make_config(d, E, fast=fast)
    A, ids = cfg.num_agents, _abi.num_actions(cfg)
    duration = int(d["duration"] * d["policy_frequency"])
    spawn = {"ego_spacing": float(d["ego_spacing"]), "vehicles_density": float(d["vehicles_density"])}
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    rng = np.random.default_rng(0)
    acts = [torch.from_numpy(rng.integers(0, ids, size=(E, A)).astype(np.int32)).to(dev) for _ in range(16)]

    def planes():
        return {"obs": torch.empty((E, A, *_abi.obs_shape(cfg)), dtype=torch.float32, device=dev),
                "reward": torch.empty((E, A), dtype=torch.float64, device=dev), "terminated": torch.empty(E, dtype=torch.uint8, device=dev),
                "truncated": torch.empty(E, dtype=torch.uint8, device=dev), "speed": torch.empty((E, A), dtype=torch.float64, device=dev),
                "crashed": torch.empty((E, A), dtype=torch.uint8, device=dev)}

    engines = {k: Engine(cfg, device=0, stream=stream.cuda_stream) for k in ("next", "same")}
    out = {k: planes() for k in engines}
    final = {"obs": torch.zeros_like(out["same"]["obs"]), "speed": torch.zeros_like(out["same"]["speed"]),
             "crashed": torch.zeros_like(out["same"]["crashed"]), "mask": torch.zeros(E, dtype=torch.uint8, device=dev),
             "action_mask": torch.zeros((E, A, ids), dtype=torch.uint8, device=dev),
             "final_action_mask": torch.zeros((E, A, ids), dtype=torch.uint8, device=dev)}
    torch.cuda.synchronize()
    k = {"next": 0, "same": 0}

    def ptrs(which):
        return [out[which][f].data_ptr() for f in ("obs", "reward", "terminated", "truncated", "speed", "crashed")]

    def next_step():
        engines["next"].step_device(acts[k["next"] % 16].data_ptr(), *ptrs("next"))
        k["next"] += 1

    def same_step(masks=False):
        engines["same"].step_same_step_device(acts[k["same"] % 16].data_ptr(), *ptrs("same"), final["obs"].data_ptr(), final["speed"].data_ptr(),
                                              final["crashed"].data_ptr(), final["mask"].data_ptr(),
                                              final["action_mask"].data_ptr() if masks else 0,
                                              final["final_action_mask"].data_ptr() if masks else 0)
        k["same"] += 1

    def timed(fn, n):
        with torch.cuda.stream(stream):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            for _ in range(n):
                fn()
            t1.record(stream)
        t1.synchronize()
        return 1000.0 * t0.elapsed_time(t1) / n

    # reset alike; spread the time limits over the calls of one episode length
    seeds = np.arange(E, dtype=np.uint64) + np.uint64(12345)
    for eng in engines.values():
        eng.reset(seeds=seeds, **spawn)
        eng.set_autoreset(True, base_seed=99, **spawn)
    for j in range(duration):
        next_step()
        same_step()
        mask = ((np.arange(E) % duration) == j).astype(np.uint8)
        for eng in engines.values():
            eng.reset(seeds=seeds + np.uint64(1000 * (j + 1)), mask=mask, **spawn)
    for _ in range(max(a.warmup, 100)):  # (past the engine's own selection of the issue-priority turn: 85 timed launches per stage)
        next_step()
        same_step()
    torch.cuda.synchronize()

    kinds = {"next_step": next_step, "same_step": same_step, "same_step_masks": lambda: same_step(True)}
    us = {n: [] for n in kinds}
    for _ in range(a.rounds):
        for n, fn in kinds.items():
            us[n].append(timed(fn, a.launches))
    # the rate of episode ends, counted in a pass of its own (the count is torch kernels on the stream: not inside a sample)
    rows = {}
    for n, fn in kinds.items():
        which = "next" if n == "next_step" else "same"
        total = torch.zeros((), dtype=torch.int64, device=dev)
        with torch.cuda.stream(stream):
            for _ in range(a.launches):
                fn()
                total.add_((out[which]["terminated"] | out[which]["truncated"]).sum())
        stream.synchronize()
        rows[n] = int(total.item())
    # the step kernel's own dispatch time in either mode
    prof = {}
    for which, fn in (("next", next_step), ("same", same_step)):
        engines[which].profile_enable(1)
        timed(fn, a.launches)
        ms, n = engines[which].profile_read()
        engines[which].profile_enable(0)
        prof[which] = 1000.0 * ms / max(n, 1)
    for eng in engines.values():
        eng.close()
    med = {n: float(np.median(v)) for n, v in us.items()}
    calls = a.launches
    useful = {}
    for n in kinds:
        ends = float(rows[n])
        share = ends / (calls * E)
        # next-step: every ending is followed by one re-spawn row, which is not a useful step
        useful[n] = {"ended_rows_per_call": round(ends / calls, 2), "ended_share": round(share, 5),
                     "us_per_useful_env_step": round(med[n] / (E * (1.0 - share)) if n == "next_step" else med[n] / E, 6)}
    return {"shape": f"{E} x {env_id} x {cfg.num_vehicles} vehicles, {cfg.lanes_count} lanes, duration {duration} steps",
            "launches_per_round": a.launches, "rounds": a.rounds,
            "us_per_call": {n: round(v, 2) for n, v in med.items()},
            "us_per_call_rounds": {n: [round(x, 2) for x in v] for n, v in us.items()},
            "spread_us": {n: round(max(v) - min(v), 2) for n, v in us.items()},
            "same_step_minus_next_step_us": round(med["same_step"] - med["next_step"], 2),
            "masks_add_us": round(med["same_step_masks"] - med["same_step"], 2),
            "step_kernel_dispatch_us": {"next_step": round(prof["next"], 2), "same_step": round(prof["same"], 2)},
            "stash_and_respawn_add_us": round(med["same_step"] - prof["same"], 2),
            "useful": useful}


def frontend_section(a, torch, name) -> dict:
    from highwayenv_amd.vector import HighwayVectorEnv
    env_id, _, over = SHAPES[name]
    E = a.envs
    rng = np.random.default_rng(1)
    host_acts = [rng.integers(0, 5, size=E).astype(np.int32) for _ in range(16)]
    dev_acts = [torch.from_numpy(x).cuda() for x in host_acts]
    make = {"torch NextStep": lambda: HighwayVectorEnv(env_id, E, config=dict(over), output="torch"),
            "torch SameStep": lambda: HighwayVectorEnv(env_id, E, config=dict(over), output="torch", autoreset_mode="SameStep"),
            "numpy SameStep": lambda: HighwayVectorEnv(env_id, E, config=dict(over), autoreset_mode="SameStep")}
    venvs = {n: f() for n, f in make.items()}
    for v in venvs.values():
        v.reset(seed=0)

    def run(n, v, steps):
        acts = host_acts if n.startswith("numpy") else dev_acts
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            v.step(acts[i % 16])
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0) / steps

    steps = max(a.launches // 2, 50)
    for n, v in venvs.items():
        run(n, v, 60)  # (through the first time limit: the rate of episode ends is the natural one afterwards only on average)
    wall = {n: [] for n in venvs}
    for _ in range(a.rounds):
        for n, v in venvs.items():
            wall[n].append(run(n, v, steps))
    for v in venvs.values():
        v.close()
    return {"steps_per_round": steps, "wall_us_per_step": {n: round(float(np.median(v)), 2) for n, v in wall.items()},
            "wall_us_per_step_rounds": {n: [round(x, 2) for x in v] for n, v in wall.items()}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=310)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--configs", default="fast,v0")
    ap.add_argument("--skip-frontends", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    from highwayenv_amd import build
    res = {"device": None, "kernel_source_hash": build.kernel_source_hash(), "configs": {}}
    for name in a.configs.split(","):
        sec = {"device_time": device_section(a, torch, name)}
        if not a.skip_frontends:
            sec["front_ends"] = frontend_section(a, torch, name)
        res["configs"][name] = sec
    res["device"] = torch.cuda.get_device_name(0)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
