#!/usr/bin/env python3
"""What the action mask costs at one shape (default: 4096 x highway-fast-v0 x 51 vehicles, 4 lanes): device time per launch of the
mask kernel alone (hwy_action_mask_device), of the step kernel of the same build on the same device and state (hwy_step_device)
and of a step with the mask launched behind it -- what HighwayVectorEnv(output="torch", action_masks=True) enqueues per step --
and the wall time per step of that front end with and without action_masks; then (b) plan_opd(50, 0.7) masked against unmasked
and plan_lookahead(2) masked against unmasked at the shapes of profiles/opd.md (4096 x highway-fast-v0 x 51 vehicles, device spawn
with seed 0, five random steps into the episodes), the two alternating call by call, each call between two events on the engine's
stream; and (c) 4096 full episodes from the same seeded start states driven by the masked and by the unmasked plan at budget 50:
return, crash rate, episode length and the mean depth of the greedy sequence.

    python tools/mask_bench.py [--envs 4096] [--vehicles 50] [--lanes 4] [--launches 300] [--rounds 5] [--out profiles/mask_bench.json]

Each sample is `--launches` back-to-back launches on the engine's stream between two events recorded on that stream (the elapsed
time divided by the number of launches: kernel time plus the gap between consecutive dispatches), after a warm-up that also steps
the engine into the middle of its episodes (and past its own selection of the issue-priority turn).  The kinds alternate in
`--rounds` rounds, so that clock drift hits them alike; every round is reported, the summary is the median.  The front-end samples
are a host clock around `--launches` steps that end in a device synchronise.  Prints one JSON line and, with --out, writes it."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--vehicles", type=int, default=50)
    ap.add_argument("--lanes", type=int, default=4)
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--budget", type=int, default=50)
    ap.add_argument("--gamma", type=float, default=0.7)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--skip-opd", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    from highwayenv_amd import _abi, build, spawn
    from highwayenv_amd.engine import Engine
    from highwayenv_amd.vector import HighwayVectorEnv

    E = a.envs
    d = _abi.highway_fast_default_config()
    d.update({"vehicles_count": a.vehicles, "lanes_count": a.lanes})
    cfg = _abi.make_config(d, E, fast=True)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    eng = Engine(cfg, device=0, stream=stream.cuda_stream)
    eng.set_state(spawn.spawn_reference_stream(cfg, np.arange(E), d["ego_spacing"], d["vehicles_density"]))
    eng.set_autoreset(True, base_seed=1, ego_spacing=d["ego_spacing"], vehicles_density=d["vehicles_density"])
    rng = np.random.default_rng(0)
    acts = [torch.from_numpy(rng.integers(0, 5, size=(E, 1)).astype(np.int32)).to(dev) for _ in range(16)]
    out = (torch.empty((E, 1, *_abi.obs_shape(cfg)), dtype=torch.float32, device=dev), torch.empty((E, 1), dtype=torch.float64, device=dev),
           torch.empty(E, dtype=torch.uint8, device=dev), torch.empty(E, dtype=torch.uint8, device=dev))
    mask = torch.empty((E, 1, 5), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    k = [0]

    def step():
        eng.step_device(acts[k[0] % 16].data_ptr(), *(t.data_ptr() for t in out))
        k[0] += 1

    def mask_only():
        eng.action_mask_device(mask.data_ptr())

    def step_and_mask():
        step()
        mask_only()

    kinds = {"step": step, "mask": mask_only, "step_and_mask": step_and_mask}

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
    for fn in kinds.values():
        timed(fn, 50)
    us = {name: [] for name in kinds}
    for _ in range(a.rounds):
        for name, fn in kinds.items():
            us[name].append(timed(fn, a.launches))
    available = mask.float().mean(dim=(0, 1)).cpu().numpy().round(4).tolist()
    eng.close()

    # the vector front end: wall time per step, masks off and on, alternating
    venvs = {on: HighwayVectorEnv("highway-fast-v0", E, config={"vehicles_count": a.vehicles, "lanes_count": a.lanes}, output="torch",
                                  action_masks=on) for on in (False, True)}
    for v in venvs.values():
        v.reset(seed=0)
    wall = {False: [], True: []}

    def run(v, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            v.step(acts[i % 16][:, 0])
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0) / n

    for v in venvs.values():
        run(v, a.warmup)
    for _ in range(a.rounds):
        for on, v in venvs.items():
            wall[on].append(run(v, a.launches))
    for v in venvs.values():
        v.close()
    med = {n: float(np.median(v)) for n, v in us.items()}
    res = {"shape": f"{E} x highway-fast-v0 x {a.vehicles + 1} vehicles, {a.lanes} lanes", "launches_per_round": a.launches, "rounds": a.rounds,
           "us_per_launch": {n: round(v, 2) for n, v in med.items()},
           "us_per_round": {n: [round(x, 2) for x in v] for n, v in us.items()},
           "mask_over_step": round(med["mask"] / med["step"], 4),
           "step_and_mask_minus_step_us": round(med["step_and_mask"] - med["step"], 2),
           "vector_env_wall_us_per_step": {"action_masks=False": round(float(np.median(wall[False])), 2),
                                           "action_masks=True": round(float(np.median(wall[True])), 2)},
           "vector_env_wall_us_per_round": {"action_masks=False": [round(x, 2) for x in wall[False]],
                                            "action_masks=True": [round(x, 2) for x in wall[True]]},
           "bytes_read_per_row": 4 + 2 * 8, "bytes_written_per_row": 5, "available_share_per_column": available,
           "kernel_source_hash": build.kernel_source_hash(), "device": torch.cuda.get_device_name(0)}
    if not a.skip_opd:
        res["opd"] = opd_section(a, torch, dev)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res))


def opd_section(a, torch, dev) -> dict:
    from highwayenv_amd.vector import HighwayVectorEnv
    E = a.envs
    stream = torch.cuda.Stream(device=dev)
    config = {"vehicles_count": a.vehicles}   # (3 lanes: the shape of profiles/opd.md)

    def make():
        return HighwayVectorEnv("highway-fast-v0", E, config=config, output="torch", autoreset_mode="Disabled", stream=stream)

    def one(fn):
        with torch.cuda.stream(stream):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            fn()
            t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1)

    def alternate(kinds, repeats, warmup=5):
        samples = {k: [] for k in kinds}
        for it in range(warmup + repeats):
            for k, fn in kinds.items():
                ms = one(fn)
                if it >= warmup:
                    samples[k].append(ms)
        return samples

    venv = make()
    with torch.cuda.stream(stream):
        venv.reset(seed=0)
        gen = torch.Generator(device=dev).manual_seed(0)
        for _ in range(5):   # into the middle of the episodes
            venv.step(torch.randint(0, 5, (E,), dtype=torch.int32, device=dev, generator=gen))
    out = {"envs": E, "budget": a.budget, "gamma": a.gamma, "expansions": a.budget // 5}
    with torch.cuda.stream(stream):
        _, d0 = venv.plan_opd(a.budget, a.gamma, return_details=True)
        exp0, depth0 = float(d0["expanded"].double().mean()), float((d0["sequence"] >= 0).sum(dim=1).double().mean())
        _, d1 = venv.plan_opd(a.budget, a.gamma, return_details=True, masked=True)
        exp1, depth1 = float(d1["expanded"].double().mean()), float((d1["sequence"] >= 0).sum(dim=1).double().mean())
        unavailable = float(1.0 - venv.env._engine.action_mask().mean())
    stream.synchronize()
    s = alternate({"unmasked": lambda: venv.plan_opd(a.budget, a.gamma), "masked": lambda: venv.plan_opd(a.budget, a.gamma, masked=True)},
                  a.repeats)
    out["plan_opd_ms"] = {k: {"median": float(np.median(v)), "min": min(v), "max": max(v), "samples": [round(x, 4) for x in v]} for k, v in s.items()}
    out["plan_opd_masked_minus_unmasked_ms"] = float(np.median(s["masked"]) - np.median(s["unmasked"]))
    out["expanded_mean"] = {"unmasked": exp0, "masked": exp1}
    out["sequence_depth_mean"] = {"unmasked": depth0, "masked": depth1}
    out["unavailable_share_at_the_root"] = unavailable
    s = alternate({"unmasked": lambda: venv.plan_lookahead(2, gamma=a.gamma), "masked": lambda: venv.plan_lookahead(2, gamma=a.gamma, masked=True)},
                  a.repeats)
    out["plan_lookahead2_ms"] = {k: {"median": float(np.median(v)), "min": min(v), "max": max(v), "samples": [round(x, 4) for x in v]} for k, v in s.items()}
    venv.close()

    # (c) what the masks change per episode: the same seeded start states for both
    out["episodes"] = {}
    for name, masked in (("unmasked", False), ("masked", True)):
        v = make()
        with torch.cuda.stream(stream):
            v.reset(seed=1000)
            ret = torch.zeros(E, dtype=torch.float64, device=dev)
            length = torch.zeros(E, dtype=torch.int32, device=dev)
            depth = torch.zeros(E, dtype=torch.float64, device=dev)
            alive = torch.ones(E, dtype=torch.bool, device=dev)
            crashed = torch.zeros(E, dtype=torch.bool, device=dev)
            for _ in range(int(v.env.config["duration"] * v.env.config["policy_frequency"])):
                action, det = v.plan_opd(a.budget, a.gamma, return_details=True, masked=masked)
                depth += torch.where(alive, (det["sequence"] >= 0).sum(dim=1).double(), torch.zeros_like(depth))
                _, r, te, tr, info = v.step(action)
                ret += torch.where(alive, r, torch.zeros_like(r))
                length += alive.int()
                crashed |= alive & info["crashed"]
                alive = alive & ~(te | tr)
        stream.synchronize()
        out["episodes"][name] = {"mean_return": float(ret.mean()), "mean_length": float(length.double().mean()),
                                 "crashed_fraction": float(crashed.double().mean()),
                                 "mean_sequence_depth": float((depth.sum() / length.double().sum())), "still_running": int(alive.sum())}
        v.close()
    return out


if __name__ == "__main__":
    main()
