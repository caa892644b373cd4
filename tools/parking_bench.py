#!/usr/bin/env python3
"""Time the parking advance kernel (csrc/hwy_park.h: hwy_park_advance_kernel) on the GPU: per policy step, for E environments,
``vehicles_count`` parked vehicles and ``k_steps`` steps per launch; next to each time the bytes a launch moves and the HBM time
they imply.  Needs a GPU (there is no fallback).  One JSON line per shape; ``--out`` also writes them to a file.

    python tools/parking_bench.py [--envs 4096 65536] [--vehicles 0 10] [--k 1 16] [--launches 200] [--repeats 5] [--out FILE]
    python tools/parking_bench.py --plan [--plan-shape 4096 64 8 3] [--plan-launches 200] [--repeats 5] [--out FILE]   (bench_plan)

Method: device tensors in and out (``hwy_park_advance_device``: no host round trip), a device reset, ``--warmup`` launches, then
``--repeats`` windows of ``--launches`` back-to-back launches, each window closed by a stream synchronise and timed by the host
clock around it; the median window is reported with the spread.  Actions are small random throttle and steering, so that episodes
last; auto-reset is on, as in training.  Back-to-back launches on one stream: the figure is the launch-to-launch time, which at
small E is the launch latency and not the kernel's own run time.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8.0e12  # MI355X: 8 TB/s peak


def launch_bytes(E: int, k_steps: int) -> int:
    """Bytes one launch moves on the common path (no struck vehicle: the parked planes and the list order are not touched): the ego
    planes (9 f64) and the integer planes (8 i32) read and written, K float32 action pairs read, the last step's observation (18
    float32), reward (f64) and flag byte written."""
    return E * (2 * (9 * 8 + 8 * 4) + k_steps * 8 + 18 * 4 + 8 + 1)


def bench_plan(args) -> list:
    """``--plan``: one search of every environment at ``parking-parked-v0`` (E, B, K, I = ``--plan-shape``), three ways.
    ``plan_cem``: ``hwy_park_cem_plan_device`` (csrc/hwy_park_cem.h, one launch per search) into device tensors, ``--warmup``
    searches, then ``--repeats`` windows of ``--plan-launches`` back-to-back searches, each closed by a stream synchronise.
    ``plan_mppi``: ``hwy_park_mppi_plan_device`` (csrc/hwy_park_mppi.h) from the same parents with the same seed, temperature 0.1,
    timed the same way; its windows alternate with ``plan_cem``'s, so that the two share whatever else the machine is doing.
    ``doors``: the same search built from ``get_state`` / ``set_state`` / ``rollout``: per iteration the parent state tiled into a
    second engine of E * B environments, host sampling (NumPy normals around the mean), one K-step rollout, the fold and the refit on
    the host; one warm-up search, then ``--repeats`` searches timed one by one by the host clock (every call synchronises)."""
    import numpy as np
    import torch
    from highwayenv_amd import build, parking
    E, B, K, I = args.plan_shape
    M, gamma = 8, 0.9
    kernels = build.kernel_resources()
    cfg = dict(parking.parking_default_config(), vehicles_count=10)
    eng = parking.ParkEngine(parking.make_park_config(cfg, E, base_seed=1))
    eng.reset()
    cem = parking.park_cem_params(B, M, I, K, gamma, 0.5, 0.05, 1.0, 7)
    mppi = parking.park_mppi_params(B, I, K, gamma, 0.5, 0.1, args.mppi_beta, 1.0, 7)
    action = torch.empty((E, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    # the two planners side by side: same parents, same white noise, their windows alternated within one run
    legs = {"plan_cem": (lambda: eng.cem_plan_device(cem, action.data_ptr()), "hwy::hwy_park_cem_kernel<true>"),
            "plan_mppi": (lambda: eng.mppi_plan_device(mppi, action.data_ptr()), "hwy::hwy_park_mppi_kernel<false>")}
    for search, _ in legs.values():
        for _ in range(args.warmup):
            search()
    eng.sync()
    windows = {what: [] for what in legs}
    for _ in range(args.repeats):
        for what, (search, _) in legs.items():
            t0 = time.perf_counter()
            for _ in range(args.plan_launches):
                search()
            eng.sync()
            windows[what].append((time.perf_counter() - t0) / args.plan_launches)
    lines = []
    for what, (_, kernel) in legs.items():
        w, res = sorted(windows[what]), kernels[kernel]
        lines.append({"what": what, "envs": E, "population": B, "horizon": K, "iterations": I, "vehicles_count": 10,
                      "ms_per_search": w[len(w) // 2] * 1e3, "ms_per_search_min": w[0] * 1e3, "ms_per_search_max": w[-1] * 1e3,
                      "env_steps_per_s": E * B * K * I / w[len(w) // 2], "vgpr": res["vgpr"], "vgpr_spill": res["vgpr_spill"],
                      "scratch": res["scratch"], "lds_static": res["lds"], "lds_dynamic": 8 * B * K})
    lines[1]["beta"] = args.mppi_beta

    work = parking.ParkEngine(parking.make_park_config(cfg, E * B))
    rng = np.random.default_rng(7)

    def doors_search():
        parent = eng.get_state()
        mean, std = np.zeros((E, K, 2)), np.full((E, K, 2), 0.5)
        for _ in range(I):
            work.set_state({k: np.repeat(v, B, axis=0) for k, v in parent.items()})
            z = rng.standard_normal((E, B, K, 2))
            z[:, 0] = 0.0
            x = np.clip(mean[:, None] + std[:, None] * z, -1.0, 1.0).astype(np.float32)
            _, _, _, sr, sf = work.advance(np.ascontiguousarray(x.reshape(E * B, K, 2).transpose(1, 0, 2)), per_step=True)
            ended = (sf & (parking.S_TERMINATED | parking.S_TRUNCATED)) != 0
            alive = np.vstack([np.ones((1, E * B), bool), ~np.logical_or.accumulate(ended, axis=0)[:-1]])
            ret = ((gamma ** np.arange(K))[:, None] * sr * alive).sum(0).reshape(E, B)
            elite = np.take_along_axis(x, np.argsort(-ret, axis=1, kind="stable")[:, :M, None, None], axis=1).astype(np.float64)
            mean, std = elite.mean(1), np.maximum(0.05, elite.std(1))
        return mean

    doors_search()
    times = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        doors_search()
        times.append(time.perf_counter() - t0)
    times.sort()
    lines.append({"what": "doors", "envs": E, "population": B, "horizon": K, "iterations": I, "vehicles_count": 10,
                  "ms_per_search": times[len(times) // 2] * 1e3, "ms_per_search_min": times[0] * 1e3, "ms_per_search_max": times[-1] * 1e3,
                  "env_steps_per_s": E * B * K * I / times[len(times) // 2]})
    work.close()
    eng.close()
    for line in lines:
        print(json.dumps(line), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plan", action="store_true", help="time a search instead (plan_cem beside plan_mppi, and the CEM search through the doors)")
    ap.add_argument("--plan-shape", type=int, nargs=4, default=[4096, 64, 8, 3], metavar=("E", "B", "K", "I"))
    ap.add_argument("--plan-launches", type=int, default=200)
    ap.add_argument("--mppi-beta", type=float, default=0.0, help="the noise colouring of the plan_mppi leg")
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--vehicles", type=int, nargs="+", default=[0, 10])
    ap.add_argument("--k", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("parking_bench needs a GPU: nothing is measured without one")
    from highwayenv_amd import build, parking
    res = build.kernel_resources()["hwy::hwy_park_advance_kernel<256>"]
    lines = bench_plan(args) if args.plan else []
    for E in [] if args.plan else args.envs:
        for vc in args.vehicles:
            cfg = dict(parking.parking_default_config(), vehicles_count=vc)
            eng = parking.ParkEngine(parking.make_park_config(cfg, E, autoreset=True, base_seed=1))
            eng.reset()
            for K in args.k:
                g = torch.Generator(device="cuda").manual_seed(E + vc + K)
                actions = (torch.rand((K, E, 2), device="cuda", generator=g) - 0.5) * 0.6
                obs = torch.empty((E, 3, 6), dtype=torch.float32, device="cuda")
                reward = torch.empty(E, dtype=torch.float64, device="cuda")
                flags = torch.empty(E, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                ptrs = (actions.data_ptr(), obs.data_ptr(), reward.data_ptr(), flags.data_ptr())
                for _ in range(args.warmup):
                    eng.advance_device(K, *ptrs)
                eng.sync()
                windows = []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    for _ in range(args.launches):
                        eng.advance_device(K, *ptrs)
                    eng.sync()
                    windows.append((time.perf_counter() - t0) / args.launches)
                windows.sort()
                per_launch = windows[len(windows) // 2]
                nbytes = launch_bytes(E, K)
                lines.append({"envs": E, "vehicles_count": vc, "k_steps": K, "us_per_launch": per_launch * 1e6,
                              "us_per_policy_step": per_launch * 1e6 / K, "us_per_launch_min": windows[0] * 1e6,
                              "us_per_launch_max": windows[-1] * 1e6, "env_steps_per_s": E * K / per_launch,
                              "bytes_per_launch": nbytes, "hbm_us_per_launch": nbytes / HBM_BYTES_PER_S * 1e6,
                              "vgpr": res["vgpr"], "vgpr_spill": res["vgpr_spill"], "scratch": res["scratch"]})
                print(json.dumps(lines[-1]), flush=True)
            eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
