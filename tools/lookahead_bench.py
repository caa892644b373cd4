#!/usr/bin/env python3
"""What a device-side fork and a simulator-based plan cost at one shape (default: 4096 x highway-fast-v0 x 51 vehicles):

 (a) hwy_fork_device at B = 25 and B = 125 branches per environment: device time per call and bytes written per second, next to a
     device-to-device copy (hipMemcpyDtoDAsync, through torch's ``copy_``) of the same byte count in the same run -- the yardstick
     a plain copy gives;
 (b) plan_lookahead(depth=2, horizon=4) per call on the device, split into fork / rollout / score (events between the three);
 (c) the same plan through the route that existed before -- get_state -> np.repeat -> set_state -> rollout (host pointers) -> numpy
     fold -- by the host clock, on the same box; and the ratio (c) / (b).

    python tools/lookahead_bench.py [--envs 4096] [--vehicles 50] [--repeats 20] [--warmup 5] [--host-repeats 3] [--out FILE.json]

One process; every device sample is one call between two events recorded on the engine's stream, after `--warmup` calls; the
summary of each kind is the median of `--repeats` samples (the samples are reported too).  Prints one JSON line and, with --out,
writes it."""
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
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--gamma", type=float, default=0.9)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    from highwayenv_amd import _abi, build, spawn
    from highwayenv_amd.engine import Engine

    E = a.envs
    d = _abi.highway_fast_default_config()
    d.update({"vehicles_count": a.vehicles})
    cfg = _abi.make_config(d, E, fast=True)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    parent = Engine(cfg, device=0, stream=stream.cuda_stream)
    parent.set_state(spawn.spawn_reference_stream(cfg, np.arange(E), d["ego_spacing"], d["vehicles_density"]))
    parent.set_autoreset(False)
    rng = np.random.default_rng(0)
    for _ in range(5):   # into the middle of the episodes
        parent.step(rng.integers(0, 5, size=(E, 1)).astype(np.int32))
    pitch = (cfg.num_vehicles + 7) // 8 * 8
    env_bytes = pitch * (9 * 8 + 4) + 8 + 4 + 1   # what the fork writes per destination environment

    def with_envs(n):
        c = _abi.HwyConfig.from_buffer_copy(bytes(cfg))
        c.num_envs = n
        return c

    def timed(fns, repeats, warmup):
        """Median device ms of every stage of `fns` (run back to back on the stream), and the samples."""
        samples = [[] for _ in fns]
        for it in range(warmup + repeats):
            with torch.cuda.stream(stream):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)]
                ev[0].record(stream)
                for fn, e in zip(fns, ev[1:]):
                    fn()
                    e.record(stream)
            ev[-1].synchronize()
            if it >= warmup:
                for k in range(len(fns)):
                    samples[k].append(ev[k].elapsed_time(ev[k + 1]))
        return [float(np.median(s)) for s in samples], samples

    result = {"what": "tools/lookahead_bench.py", "envs": E, "vehicles": cfg.num_vehicles, "pitch": pitch,
              "kernel_source_hash": build.kernel_source_hash(), "device": torch.cuda.get_device_name(0), "fork": {}}

    # ---- (a) the fork next to a plain copy of the same bytes ---------------------------------------------------------------------
    for B in (25, 125):
        child = Engine(with_envs(E * B), device=0, stream=stream.cuda_stream)
        child.set_autoreset(False)
        nbytes = E * B * env_bytes
        src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        (fork_ms, copy_ms), (fork_s, copy_s) = timed([lambda: child.fork_device(parent, B), lambda: dst.copy_(src, non_blocking=True)],
                                                     a.repeats, a.warmup)
        result["fork"][f"B{B}"] = {"branch_envs": E * B, "bytes_written": nbytes, "fork_ms": fork_ms, "fork_GBps": nbytes / fork_ms / 1e6,
                                   "memcpy_dtod_ms": copy_ms, "memcpy_dtod_GBps": nbytes / copy_ms / 1e6,
                                   "fork_ms_samples": fork_s, "memcpy_dtod_ms_samples": copy_s}
        del src, dst
        child.close()

    # ---- (b) plan_lookahead(2, horizon=4) on the device ----------------------------------------------------------------------------
    B, K, n = 25, 4, E * 25
    child = Engine(with_envs(n), device=0, stream=stream.cuda_stream)
    child.set_autoreset(False)
    b = np.arange(B)
    table = np.ones((B, K), np.int32)
    table[:, 0], table[:, 1] = b // 5, b % 5
    planes = np.ascontiguousarray(np.broadcast_to(table.T[:, None, :], (K, E, B)).reshape(K, n, 1))
    acts = torch.from_numpy(planes).to(dev)
    obs = torch.empty((K, n, 1, *_abi.obs_shape(cfg)), dtype=torch.float32, device=dev)
    rew = torch.empty((K, n, 1), dtype=torch.float64, device=dev)
    term, trunc = torch.empty((K, n), dtype=torch.uint8, device=dev), torch.empty((K, n), dtype=torch.uint8, device=dev)
    ret = torch.empty((E, B, 1), dtype=torch.float64, device=dev)
    q = torch.empty((E, 5), dtype=torch.float64, device=dev)
    best, branch = torch.empty(E, dtype=torch.int32, device=dev), torch.empty((E, 1), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    stages = [lambda: child.fork_device(parent, B),
              lambda: child.rollout_device(K, acts.data_ptr(), obs.data_ptr(), rew.data_ptr(), term.data_ptr(), trunc.data_ptr()),
              lambda: child.score_device(K, B, a.gamma, acts.data_ptr(), rew.data_ptr(), term.data_ptr(), trunc.data_ptr(), ret.data_ptr(),
                                         q.data_ptr(), best.data_ptr(), branch.data_ptr())]
    (fork_ms, roll_ms, score_ms), samples = timed(stages, a.repeats, a.warmup)
    totals = [sum(s[k] for s in samples) for k in range(a.repeats)]
    device_best = best.cpu().numpy()
    result["plan_device"] = {"depth": 2, "horizon": K, "branches": B, "fork_ms": fork_ms, "rollout_ms": roll_ms, "score_ms": score_ms,
                             "total_ms": float(np.median(totals)), "total_ms_samples": totals}

    # ---- (c) the same plan through the host route ----------------------------------------------------------------------------------
    host = Engine(with_envs(n), device=0)
    host.set_autoreset(False)
    index = np.arange(n) // B
    host_ms, host_split = [], []
    for _ in range(a.host_repeats):
        t0 = time.perf_counter()
        st = parent.get_state()
        t1 = time.perf_counter()
        rep = {k: np.ascontiguousarray(v[index]) for k, v in st.items()}
        t2 = time.perf_counter()
        host.set_state(rep)
        t3 = time.perf_counter()
        _, r, te, tr, _ = host.rollout(planes)
        t4 = time.perf_counter()
        g, alive, disc = np.zeros(n), np.ones(n, bool), 1.0
        for k in range(K):
            g = np.where(alive, g + disc * r[k, :, 0], g)
            alive &= ~(te[k] | tr[k])
            disc *= a.gamma
        qh = g.reshape(E, 5, 5).max(axis=2)   # branch b starts with action b // 5
        host_best = np.argmax(qh, axis=1)
        t5 = time.perf_counter()
        host_ms.append(1000 * (t5 - t0))
        host_split.append({"get_state_ms": 1000 * (t1 - t0), "repeat_ms": 1000 * (t2 - t1), "set_state_ms": 1000 * (t3 - t2),
                           "rollout_ms": 1000 * (t4 - t3), "fold_ms": 1000 * (t5 - t4)})
    assert np.array_equal(host_best, device_best), "the two routes disagree on the plan"
    k = int(np.argsort(host_ms)[len(host_ms) // 2])
    result["plan_host_route"] = {"total_ms": host_ms[k], "total_ms_samples": host_ms, **host_split[k]}
    result["host_over_device"] = host_ms[k] / result["plan_device"]["total_ms"]
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
