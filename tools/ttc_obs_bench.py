#!/usr/bin/env python3
"""What the TimeToCollision observation costs on the device (default shape: 4096 x highway-fast-v0 x 51 vehicles, horizon 10 s).

    python tools/ttc_obs_bench.py [--parent-root DIR] [--processes 3] [--rounds 5] [--launches 2000] [--out FILE.json] [--md FILE.md]

Three questions, one JSON line (and, with ``--md``, the table of profiles/ttc_observation.md):
  (a) baseline step    ``hwy_step_device`` of this checkout and of ANOTHER checkout (``--parent-root``: the parent commit, built) in
                       the same session.  No step kernel changed, so the two must agree within the spread the run itself reports:
                       ``step_process_ranges_meet`` (gate() has the rule); exit status 3 where they do not.
  (b) step + window    ``hwy_step_device`` followed by ``hwy_ttc_observe_device`` ("step_window"), and the SameStep one-call forms
                       ``hwy_step_same_step_device`` ("same_step") and ``hwy_step_same_step_ttc_device`` ("same_step_window").
  (c) kernel alone     ``hwy_ttc_observe_device`` ("window_kernel") against ``hwy_ttc_grid_device`` ("grid_kernel"), the full-grid
                       kernel a user had before (plus a host-side window), on the same state.
Numbers are us per call: device events around a window of ``--launches`` calls enqueued on the engine's stream and ended by a
synchronise -- what a training loop that keeps the policy on the GPU pays, launch gaps included; for (c), back-to-back launches of
one small kernel, that is the kernel's duration or the launch rate, whichever is larger (``kernel_us`` of the step variants: the
step kernel's own duration from the dispatch's timestamps, hwy_profile_*).  Every window takes the next of 16 pre-staged random
action planes, auto-reset on, after a warm-up.  The variants of one process alternate window by window.  The two checkouts' step
figures come from processes that do the same thing -- one engine, step windows only -- and alternate, in alternating order
(``--processes`` each, every one a fresh child process, one at a time).  The spread of a figure is max - min over its windows of all
processes."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ALL = "step,step_window,same_step,same_step_window,window_kernel,grid_kernel"


def measure(a) -> dict:
    """One process, one checkout (``a.root``): the windows of its variants."""
    sys.path.insert(0, a.root)
    import torch

    from highwayenv_amd import _abi, spawn
    from highwayenv_amd.engine import Engine

    E = a.envs
    d = _abi.highway_fast_default_config()
    d.update({"vehicles_count": a.vehicles, "lanes_count": a.lanes})
    cfg = _abi.make_config(d, E, fast=True)
    dev = torch.device("cuda", 0)
    variants = [v for v in a.variants.split(",") if v]
    params = _abi.ttc_params(d, horizon=a.horizon)
    T = params.time_steps
    rng = np.random.default_rng(0)
    ids = [torch.from_numpy(rng.integers(0, _abi.num_actions(cfg), size=(E, 1)).astype(np.int32)).to(dev) for _ in range(16)]
    stream = torch.cuda.Stream(device=dev)
    engines, outs, extra = {}, {}, {}
    st0 = spawn.spawn_reference_stream(cfg, np.arange(E), d["ego_spacing"], d["vehicles_density"])
    f32, f64, u8 = torch.float32, torch.float64, torch.uint8
    for name in variants:  # one engine per variant, the same shape and the same start
        eng = Engine(cfg, device=0, stream=stream.cuda_stream)
        eng.set_state(st0)
        eng.set_autoreset(True, base_seed=1, ego_spacing=d["ego_spacing"], vehicles_density=d["vehicles_density"])
        engines[name] = eng
        window = name in ("same_step_window",)
        obs = torch.empty((E, 1, 3, 3, T) if window else (E, 1, *_abi.obs_shape(cfg)), dtype=f32, device=dev)
        planes = [obs, torch.empty((E, 1), dtype=f64, device=dev), torch.empty(E, dtype=u8, device=dev), torch.empty(E, dtype=u8, device=dev)]
        if name.startswith("same_step"):
            planes += [torch.empty((E, 1), dtype=f64, device=dev), torch.empty((E, 1), dtype=u8, device=dev), torch.empty_like(obs),
                       torch.empty((E, 1), dtype=f64, device=dev), torch.empty((E, 1), dtype=u8, device=dev), torch.empty(E, dtype=u8, device=dev)]
        outs[name] = planes
        extra[name] = {"window": torch.empty((E, 1, 3, 3, T), dtype=f32, device=dev),
                       "grid": torch.empty((E, 1, cfg.num_target_speeds, cfg.lanes_count, T), dtype=f32, device=dev)}
    torch.cuda.synchronize()
    count = {name: 0 for name in variants}

    def run(name, n):
        eng, out = engines[name], [t.data_ptr() for t in outs[name]]
        w, g = extra[name]["window"].data_ptr(), extra[name]["grid"].data_ptr()
        for _ in range(n):
            k = count[name] % 16
            if name == "step":
                eng.step_device(ids[k].data_ptr(), *out)
            elif name == "step_window":
                eng.step_device(ids[k].data_ptr(), *out)
                eng.ttc_observe_device(params, w)
            elif name == "same_step":
                eng.step_same_step_device(ids[k].data_ptr(), *out)
            elif name == "same_step_window":
                eng.step_same_step_ttc_device(params, ids[k].data_ptr(), *out)
            elif name == "window_kernel":
                eng.ttc_observe_device(params, w)
            elif name == "grid_kernel":
                eng.ttc_grid_device(params, g)
            count[name] += 1

    for name in variants:  # warm-up (and the engine's own issue-priority turn selection); the kernel-alone variants observe a
        if name.endswith("_kernel"):  # state some steps into the episodes
            for k in range(20):
                engines[name].step_device(ids[k % 16].data_ptr(), *[t.data_ptr() for t in outs[name]])
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
            if name.endswith("_kernel"):
                continue
            eng = engines[name]
            eng.profile_enable(1)
            run(name, min(a.launches, 1000))
            ms, n = eng.profile_read()
            eng.profile_enable(0)
            kernel_us[name].append(1000.0 * ms / n)
    res = {"stream_us": stream_us, "kernel_us": {k: v for k, v in kernel_us.items() if v}}
    if "window_kernel" in variants and "grid_kernel" in variants:  # the same state: the window kernel gives the window of the grid
        st = engines["window_kernel"].get_state()
        engines["grid_kernel"].set_state(st)
        engines["window_kernel"].set_state(st)
        grid, win = engines["grid_kernel"].ttc_grid(params), engines["window_kernel"].ttc_observe(params)
        i = cfg.agent_index[0]
        lane, index = st["lane"][:, i], st["speed_index"][:, i]
        V, L = cfg.num_target_speeds, cfg.lanes_count
        want = np.ones_like(win)
        for a_ in range(3):
            v = np.clip(index + a_ - 1, 0, V - 1)
            for b in range(3):
                ln = lane + b - 1
                ok = (ln >= 0) & (ln < L)
                want[ok, 0, a_, b] = grid[np.flatnonzero(ok), 0, v[ok], ln[ok]]
        res["window_equals_window_of_grid"] = bool(np.array_equal(win, want))
        res["marked_share"] = round(float((win > 0).mean()), 4)
    for eng in engines.values():
        eng.close()
    return res


def summary(windows) -> dict:
    w = [x for proc in windows for x in proc]
    return {"median": round(float(np.median(w)), 2), "min": round(min(w), 2), "max": round(max(w), 2),
            "spread": round(max(w) - min(w), 2), "per_process_median": [round(float(np.median(p)), 2) for p in windows]}


def gate(res: dict) -> bool:
    """(a): the two checkouts' step figures agree within the run-to-run spread the same run reports.  A run of a checkout is one of
    its fresh processes, its figure that process's median window; the run-to-run spread of a checkout is the range of those
    medians.  The two agree when the ranges meet -- neither checkout's fastest process is slower than the other's slowest.  A step
    that got slower moves every process of this checkout and parts the ranges; one slow process (another issue-priority turn
    picked, a neighbour on the host) stretches its own range upwards only and moves nothing towards the other checkout.  Recorded
    next to it: the difference of the medians over all windows, and the stricter reading of tools/continuous_bench.py (this build's
    median no higher than the highest of the parent's windows).  Returns the verdict; main() exits with status 3 where it is False."""
    s = res["us_per_call"]["stream_us"]
    new, old = s["step"]["per_process_median"], s["parent_step"]["per_process_median"]
    for k in ("step_within_parent_spread", "run_to_run_spread_us", "step_agrees_with_parent_within_spread"):
        res.pop(k, None)
    res["step_minus_parent_stream_us"] = round(s["step"]["median"] - s["parent_step"]["median"], 2)
    res["step_process_medians_us"] = {"this": [min(new), max(new)], "parent": [min(old), max(old)]}
    res["step_process_ranges_meet"] = bool(min(new) <= max(old) and min(old) <= max(new))
    res["step_median_within_parent_windows"] = bool(s["step"]["median"] <= s["parent_step"]["max"])
    return res["step_process_ranges_meet"]


def markdown(res: dict) -> str:
    s, k = res["us_per_call"]["stream_us"], res["us_per_call"]["kernel_us"]
    rows = [("(a) `hwy_step_device`, this commit", "step"), ("(a) `hwy_step_device`, parent commit", "parent_step"),
            ("(b) `hwy_step_device` + `hwy_ttc_observe_device`", "step_window"), ("(b) `hwy_step_same_step_device` (Kinematics rows)", "same_step"),
            ("(b) `hwy_step_same_step_ttc_device`", "same_step_window"), ("(c) `hwy_ttc_observe_device` alone", "window_kernel"),
            ("(c) `hwy_ttc_grid_device` alone", "grid_kernel")]
    out = [f"Shape: {res['shape']}; {res['launches_per_window']} calls per window, {res['windows_per_process']} windows per process, "
           f"{res['processes']} processes per figure.  us per call.", "",
           "| what | stream median | min | max | spread | step kernel median |", "|---|---|---|---|---|---|"]
    for label, key in rows:
        if key in s:
            out.append(f"| {label} | {s[key]['median']} | {s[key]['min']} | {s[key]['max']} | {s[key]['spread']} | "
                       f"{k[key]['median'] if key in k else '-'} |")
    p = res.get("step_process_medians_us")
    out += ["", f"- step, this commit minus parent: {res.get('step_minus_parent_stream_us', 'not measured')} us over all windows; medians of "
                f"the processes: this commit {p['this'][0]} .. {p['this'][1]}, parent {p['parent'][0]} .. {p['parent'][1]}; the ranges meet: "
                f"{res['step_process_ranges_meet']} (median no higher than the highest of the parent's windows: "
                f"{res['step_median_within_parent_windows']})" if p else "- step of the parent commit: not measured",
            f"- the window behind the step costs {res['window_behind_step_us']} us per step; inside the SameStep call "
            f"{res['window_inside_same_step_us']} us (two observe launches and a stash of 9 T floats per row)",
            f"- window kernel against grid kernel: {res['window_kernel_minus_grid_kernel_us']} us; the window equals the window of the grid: "
            f"{res['window_equals_window_of_grid']}; share of marked cells {res['marked_share']}"]
    return "\n".join(out) + "\n"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--vehicles", type=int, default=50)
    ap.add_argument("--lanes", type=int, default=3)
    ap.add_argument("--horizon", type=float, default=10.0)
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: its hwy_step_device is measured too")
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--root", default=os.path.dirname(HERE), help=argparse.SUPPRESS)      # (child processes)
    ap.add_argument("--variants", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.variants is not None:  # a child: one checkout, one process
        print("RESULT " + json.dumps(measure(a)))
        return

    def child(root, variants):
        cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--variants", variants, "--envs", str(a.envs), "--vehicles",
               str(a.vehicles), "--lanes", str(a.lanes), "--horizon", str(a.horizon), "--launches", str(a.launches), "--warmup", str(a.warmup),
               "--rounds", str(a.rounds)]
        env = dict(os.environ)
        env.pop("HWY_ENGINE_LIB", None)
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
        if r.returncode != 0:
            raise RuntimeError(f"{root}: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        return json.loads(next(line for line in r.stdout.splitlines() if line.startswith("RESULT "))[7:])

    new, parent, both = [], [], []
    for i in range(a.processes):  # (a failing child raises: nothing more is started)
        order = [("parent", os.path.abspath(a.parent_root))] if a.parent_root else []
        order.append(("new", a.root))
        for which, root in (order if i % 2 == 0 else order[::-1]):
            (parent if which == "parent" else new).append(child(root, "step"))
        both.append(child(a.root, ALL))
        print(f"process set {i + 1} of {a.processes} done", flush=True)
    res = {"shape": f"{a.envs} x highway-fast-v0 x {a.vehicles + 1} vehicles, {a.lanes} lanes, horizon {a.horizon} s",
           "launches_per_window": a.launches, "windows_per_process": a.rounds, "processes": a.processes, "us_per_call": {}}
    for key in ("stream_us", "kernel_us"):
        res["us_per_call"][key] = {"step": summary([p[key]["step"] for p in new])}
        for name in ALL.split(","):
            if name in both[0][key]:
                res["us_per_call"][key]["beside_" + name if name == "step" else name] = summary([p[key][name] for p in both])
        if parent:
            res["us_per_call"][key]["parent_step"] = summary([p[key]["step"] for p in parent])
    s = res["us_per_call"]["stream_us"]
    res["window_behind_step_us"] = round(s["step_window"]["median"] - s["beside_step"]["median"], 2)
    res["window_inside_same_step_us"] = round(s["same_step_window"]["median"] - s["same_step"]["median"], 2)
    res["window_kernel_minus_grid_kernel_us"] = round(s["window_kernel"]["median"] - s["grid_kernel"]["median"], 2)
    res["window_equals_window_of_grid"] = all(p["window_equals_window_of_grid"] for p in both)
    res["marked_share"] = both[-1]["marked_share"]
    agree = gate(res) if parent else True
    line = json.dumps(res)
    for path, text in ((a.out, line + "\n"), (a.md, markdown(res))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)) or ".", exist_ok=True)
            with open(path, "w") as fh:
                fh.write(text)
    print(line)
    if not agree:
        sys.exit(3)


if __name__ == "__main__":
    main()
