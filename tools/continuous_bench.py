#!/usr/bin/env python3
"""What the continuous door costs: ``hwy_step_continuous_device`` (the act kernel + the step launch with no ids) against the
``DiscreteAction`` ``hwy_step_device`` on the same engine shape (default: 4096 x highway-fast-v0 x 50 vehicles, 4 lanes), and the
``DiscreteAction`` step of ANOTHER checkout of the project (``--parent-root``: the parent commit, built) in the same session.

    python tools/continuous_bench.py [--parent-root DIR] [--processes 3] [--rounds 5] [--launches 3000] [--out FILE]

Numbers (us per policy step):
  stream_us   device events around a window of ``--launches`` enqueued steps on the engine's stream, ended by a synchronise:
              what a training loop that keeps the policy on the GPU pays per step, launch gaps included;
  kernel_us   the step kernel's own duration (hwy_profile_*: the dispatch's begin / end timestamps) over a second window -- the
              act kernel is NOT in it, so stream_us(continuous) - stream_us(discrete) is what the extra dependent launch costs
              and kernel_us says whether the step kernel itself runs differently with no ids.
"act_then_discrete" is a probe, not a door: the act launch followed by the step WITH ids (whose table entry replaces the pair the act
kernel stored) -- the same results as "discrete", the same launch pattern as "continuous"; it tells a cost of running behind a small
dependent kernel from a cost of the step kernel's no-ids path.
Every window takes the next of 16 pre-staged random action planes (ids uniform over the 3 x 3 table; the continuous variant gets
the float32 grid points of the same ids, so both run the same simulation bit for bit; steering range +-0.05 rad so that the egos
meander inside the traffic), auto-reset on, after a warm-up.  The variants of one process alternate window by window
("continuous" against "beside_continuous_discrete").  The two checkouts' ``DiscreteAction`` figures ("discrete", "parent_discrete")
come from processes that do the same thing -- one engine, discrete windows only -- and alternate, in alternating order
(``--processes`` each, every one a fresh child: its own engine, its own issue-priority turn selection), so that drift and the
neighbours on the host hit them alike.
The spread of a figure is max - min over its windows of all processes.  Prints one JSON line (and writes it to ``--out``)."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def measure(a) -> dict:
    """One process, one checkout (``a.root``): the windows of its variants."""
    sys.path.insert(0, a.root)
    import torch

    from highwayenv_amd import _abi, spawn
    from highwayenv_amd.engine import Engine

    E = a.envs
    action = {"type": "DiscreteAction", "steering_range": [-0.05, 0.05]}
    d = _abi.highway_fast_default_config()
    d.update({"vehicles_count": a.vehicles, "lanes_count": a.lanes, "action": action})
    cfg = _abi.make_config(d, E, fast=True)
    dev = torch.device("cuda", 0)
    variants = [v for v in a.variants.split(",") if v]
    params = _abi.continuous_params(action) if "discrete" != a.variants else None
    rng = np.random.default_rng(0)
    host_ids = [rng.integers(0, _abi.num_actions(cfg), size=(E, 1)).astype(np.int32) for _ in range(16)]
    ids = [torch.from_numpy(i).to(dev) for i in host_ids]
    # the continuous variant drives the SAME simulation: the float32 grid points of those ids (DiscreteAction.act(i) is
    # ContinuousAction.act(all_actions[i])), so the two variants differ in the door alone, not in what the traffic does
    axis = np.linspace(-1, 1, 3, dtype=np.float32)
    floats = [torch.from_numpy(np.stack([axis[i // 3], axis[i % 3]], -1)).to(dev) for i in host_ids]  # [E, 1, 2]
    stream = torch.cuda.Stream(device=dev)
    engines, outs = {}, {}
    for name in variants:  # one engine per variant, the same shape and the same start
        eng = Engine(cfg, device=0, stream=stream.cuda_stream)
        eng.set_state(spawn.spawn_reference_stream(cfg, np.arange(E), d["ego_spacing"], d["vehicles_density"]))
        eng.set_autoreset(True, base_seed=1, ego_spacing=d["ego_spacing"], vehicles_density=d["vehicles_density"])
        engines[name] = eng
        outs[name] = tuple(t.data_ptr() for t in (
            torch.empty((E, 1, *_abi.obs_shape(cfg)), dtype=torch.float32, device=dev), torch.empty((E, 1), dtype=torch.float64, device=dev),
            torch.empty(E, dtype=torch.uint8, device=dev), torch.empty(E, dtype=torch.uint8, device=dev)))
    torch.cuda.synchronize()
    count = {name: 0 for name in variants}

    def run(name, n):
        eng, out = engines[name], outs[name]
        for _ in range(n):
            k = count[name] % 16
            if name == "continuous":
                eng.step_continuous_device(params, floats[k].data_ptr(), *out)
            elif name == "act_then_discrete":  # the act launch, then the step WITH ids (which replace what it stored): the probe
                eng.act_continuous_device(params, floats[k].data_ptr())
                eng.step_device(ids[k].data_ptr(), *out)
            else:
                eng.step_device(ids[k].data_ptr(), *out)
            count[name] += 1

    for name in variants:  # warm-up (and the engine's own issue-priority turn selection)
        run(name, a.warmup)
        engines[name].sync()
    stream_us, kernel_us = {n: [] for n in variants}, {n: [] for n in variants}
    for _ in range(a.rounds):
        for name in variants:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                start.record()
                run(name, a.launches)
                stop.record()
            stop.synchronize()
            stream_us[name].append(1000.0 * start.elapsed_time(stop) / a.launches)
        for name in variants:
            eng = engines[name]
            eng.profile_enable(1)
            run(name, min(a.launches, 1000))
            ms, n = eng.profile_read()
            eng.profile_enable(0)
            kernel_us[name].append(1000.0 * ms / n)
    res = {"stream_us": stream_us, "kernel_us": kernel_us, "prio_turn": {n: engines[n].prio_turn()[0] for n in variants}}
    for eng in engines.values():
        eng.close()
    return res


def summary(windows) -> dict:
    w = [x for proc in windows for x in proc]
    return {"median": round(float(np.median(w)), 2), "min": round(min(w), 2), "max": round(max(w), 2),
            "spread": round(max(w) - min(w), 2), "per_process_median": [round(float(np.median(p)), 2) for p in windows]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--vehicles", type=int, default=50)
    ap.add_argument("--lanes", type=int, default=4)
    ap.add_argument("--launches", type=int, default=3000)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: its DiscreteAction step is measured too")
    ap.add_argument("--out", default=None)
    ap.add_argument("--root", default=os.path.dirname(HERE), help=argparse.SUPPRESS)      # (child processes)
    ap.add_argument("--variants", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.variants is not None:  # a child: one checkout, one process
        print("RESULT " + json.dumps(measure(a)))
        return

    def child(root, variants):
        cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--variants", variants, "--envs", str(a.envs), "--vehicles",
               str(a.vehicles), "--lanes", str(a.lanes), "--launches", str(a.launches), "--warmup", str(a.warmup), "--rounds", str(a.rounds)]
        env = dict(os.environ)
        env.pop("HWY_ENGINE_LIB", None)
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(f"{root}: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        return json.loads(next(line for line in r.stdout.splitlines() if line.startswith("RESULT "))[7:])

    new, parent, both = [], [], []
    for i in range(a.processes):
        # like for like: the two checkouts' DiscreteAction figures come from processes that do the same thing (one engine, discrete
        # windows only), alternating and in alternating order; the continuous door is compared in a process of its own
        order = [("parent", os.path.abspath(a.parent_root))] if a.parent_root else []
        order.append(("new", a.root))
        for which, root in (order if i % 2 == 0 else order[::-1]):
            (parent if which == "parent" else new).append(child(root, "discrete"))
        both.append(child(a.root, "discrete,continuous,act_then_discrete"))
    res = {"shape": f"{a.envs} x highway-fast-v0 x {a.vehicles + 1} vehicles, {a.lanes} lanes", "launches_per_window": a.launches,
           "windows_per_process": a.rounds, "processes": a.processes, "us_per_step": {}}
    for key in ("stream_us", "kernel_us"):
        res["us_per_step"][key] = {"discrete": summary([p[key]["discrete"] for p in new]),
                                   "beside_continuous_discrete": summary([p[key]["discrete"] for p in both]),
                                   "continuous": summary([p[key]["continuous"] for p in both]),
                                   "act_then_discrete": summary([p[key]["act_then_discrete"] for p in both])}
        if parent:
            res["us_per_step"][key]["parent_discrete"] = summary([p[key]["discrete"] for p in parent])
    s = res["us_per_step"]["stream_us"]
    res["continuous_minus_discrete_stream_us"] = round(s["continuous"]["median"] - s["beside_continuous_discrete"]["median"], 2)
    if parent:
        res["discrete_minus_parent_stream_us"] = round(s["discrete"]["median"] - s["parent_discrete"]["median"], 2)
        # nothing existing got slower: the new build's figure is no higher than the parent's own windows reach
        res["discrete_within_parent_spread"] = bool(s["discrete"]["median"] <= s["parent_discrete"]["max"])
    res["prio_turn"] = both[-1]["prio_turn"]
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
