"""The whole control flow of an N-rank `bench.py` run on the CPU: two ranks on gloo, a stand-in engine that stamps (rank, step)
into the output planes it is handed.  What an 8-GPU node would otherwise be the first to execute -- the shard sizes, the two
alternating output buffers, `--gather-every` with a partly filled last buffer, the one-gather-per-step leg, `--scaling strong`,
the ONE JSON line with the process group's world size -- runs here (round-3 verdict item 8)."""
import ctypes as C
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeEngine:
    """Engine.step_device's contract on host memory: fills the six output planes behind the raw pointers."""

    def __init__(self, cfg, rank):
        from highwayenv_amd import _abi
        self.E, self.A, self.rank = cfg.num_envs, cfg.num_agents, rank
        self.obs_len = int(np.prod(_abi.obs_shape(cfg)))
        self.steps = 0
        self.resets_at_step = []
        self.profiled = False

    def reset(self, **kw):
        self.resets_at_step.append(self.steps)

    def set_autoreset(self, *a, **kw):
        pass

    def profile_enable(self, every):
        self.profiled = True

    def profile_read(self):
        return 0.0, 0

    def prio_turn(self):
        # HWY_FAKE_SAMPLING="40,70": rank r's engine reports "still sampling its issue-priority turns" (state 1) until it has taken
        # that many steps, "chosen" (2) afterwards; -1 = never finishes.  Unset: no selection (state 0).
        spec = os.environ.get("HWY_FAKE_SAMPLING")
        if not spec:
            return 0, 0
        need = int(spec.split(",")[self.rank])
        return 256, (1 if need < 0 or self.steps < need else 2)

    def step_device(self, d_actions, d_obs, d_reward, d_term, d_trunc, d_speed, d_crashed):
        E, A = self.E, self.A
        acts = np.ctypeslib.as_array(C.cast(d_actions, C.POINTER(C.c_int32)), (E * A,))
        assert acts.min() >= 0 and acts.max() <= 4
        self.steps += 1
        np.ctypeslib.as_array(C.cast(d_reward, C.POINTER(C.c_double)), (E * A,))[:] = 1000.0 * self.rank + self.steps
        np.ctypeslib.as_array(C.cast(d_obs, C.POINTER(C.c_float)), (E * A * self.obs_len,))[:] = self.rank
        np.ctypeslib.as_array(C.cast(d_term, C.POINTER(C.c_uint8)), (E,))[:] = self.rank + 1
        np.ctypeslib.as_array(C.cast(d_trunc, C.POINTER(C.c_uint8)), (E,))[:] = 0

    def close(self):
        pass


class CpuPlatform:
    backend = "gloo"

    def __init__(self, rank):
        self.rank = rank

    def check(self):
        pass

    def device(self, local_rank):
        return torch.device("cpu")

    def init_process_group(self, dist, rank, world, dev):
        dist.init_process_group("gloo", rank=rank, world_size=world)

    def make_engine(self, cfg, local_rank, dev):
        self.engine = FakeEngine(cfg, self.rank)
        return self.engine, None

    def synchronize(self, dev):
        pass

    def event(self):
        import time

        class Ev:
            def record(self, stream=None):
                self.t = time.perf_counter()

            def elapsed_time(self, other):
                return (other.t - self.t) * 1e3
        return Ev()


def _rank_main(rank, world, port, argv, out_path):
    os.environ.update({"RANK": str(rank), "LOCAL_RANK": str(rank), "WORLD_SIZE": str(world), "MASTER_ADDR": "127.0.0.1",
                       "MASTER_PORT": str(port)})
    sys.path.insert(0, ROOT)
    import bench
    lines = []
    plat = CpuPlatform(rank)
    outs = bench.main(argv, platform=plat, emit=lines.append)
    json.dump({"lines": lines, "steps": plat.engine.steps, "envs": plat.engine.E, "resets_at_step": plat.engine.resets_at_step,
               "profiled": plat.engine.profiled,
               "gathered_rewards": ([[float(v["reward"][0, 0]) for v in o.rank0_views(0)] for o in outs] if rank == 0 else None),
               "gathered_term": ([[int(v["terminated"][0]) for v in o.rank0_views(0)] for o in outs] if rank == 0 else None)},
              open(f"{out_path}.{rank}", "w"))


def _run(tmp_path, argv, world=2):
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    out = str(tmp_path / "rank")
    mp.spawn(_rank_main, args=(world, port, argv, out), nprocs=world, join=True)
    return [json.load(open(f"{out}.{r}")) for r in range(world)]


@pytest.mark.parametrize("sampling,chosen", [("40,90", True), ("10,-1", False)])
def test_settling_goes_on_until_the_engine_has_chosen_its_turn(tmp_path, monkeypatch, sampling, chosen):
    """bench.py's untimed settling (round 6): counted from the END of the warm-up launches, and continued -- every rank the same
    number of rounds, bounded by 20 x --settle-ms -- while ANY rank's engine is still sampling its issue-priority turns.  A cold box
    whose first launch outlasted --settle-ms used to skip the settling and time the sampling (profiles/r06_history.md section 8)."""
    monkeypatch.setenv("HWY_FAKE_SAMPLING", sampling)
    steps, warmup, repeats = 4, 5, 2
    argv = ["--gpus", "2", "--steps", str(steps), "--warmup", str(warmup), "--repeats", str(repeats), "--envs-per-gpu", "4",
            "--gather-every", "1", "--settle-ms", "2", "--no-cpu-baseline"]
    r0, r1 = _run(tmp_path, argv)
    line = r0["lines"][0]
    assert r0["steps"] == r1["steps"]  # (the settle rounds hold collectives: both ranks ran the same number)
    settle = line["settle_steps"]
    assert settle > 0 and settle % warmup == 0
    turn = line["config"]["issue_priority_turn"]
    if chosen:  # the slower rank needed 90 steps: the settling covered them although 2 ms of the fake engine are a handful of steps
        assert warmup + settle >= 90 and turn["chosen_by"] == "engine (timed its first launches)", (settle, turn)
    else:       # rank 1 never finishes: the bound (20 x 2 ms) ends the settling and the line says so (rank 0 reports its own state)
        assert turn["chosen_by"] in ("engine (timed its first launches)", "engine, still sampling")


@pytest.mark.parametrize("scaling,envs,gather_every,settle_ms", [("weak", 6, 4, 0), ("strong", 8, 1, 0), ("weak", 4, 4, 30)])
def test_two_rank_bench_control_flow_on_gloo(tmp_path, scaling, envs, gather_every, settle_ms):
    steps, warmup, repeats = 6, 3, 2   # 6 % 4 != 0: every region ends on a partly filled buffer that still has to travel
    argv = ["--gpus", "2", "--steps", str(steps), "--warmup", str(warmup), "--repeats", str(repeats), "--envs-per-gpu", str(envs),
            "--scaling", scaling, "--gather-every", str(gather_every), "--settle-ms", str(settle_ms), "--full", "--no-cpu-baseline"]
    r0, r1 = _run(tmp_path, argv)
    assert r1["lines"] == [] and len(r0["lines"]) == 1    # ONE JSON line, from rank 0
    line = r0["lines"][0]
    per_rank = envs if scaling == "weak" else envs // 2
    assert r0["envs"] == r1["envs"] == per_rank
    assert line["n_gpus"] == 2 and line["steps"] == steps and line["warmup"] == warmup and line["scaling"] == scaling
    assert line["config"]["world_size_reported_by_the_process_group"] == 2 and line["config"]["envs_per_gpu"] == per_rank
    assert line["value"] == pytest.approx(steps * per_rank * 2 / (line["ms_per_step"] * 1e-3 * steps), rel=1e-9)
    assert len(line["ms_per_step_repeats"]) == repeats and line["ms_per_step_device"] > 0
    assert "cpu_baseline" not in line and line["roofline"]["bound"] == "hbm"
    # both ranks stepped the same number of times: warm-up + regions (+ the one-gather-per-step leg when gathers are batched)
    extra = 0 if gather_every == 1 else (20 + min(steps, 300))
    extra += 10 + min(max(steps, 300), 1000)  # the kernel-timing region after the timed ones (every launch carries an event pair there; 10 uncounted launches first)
    # (the clock-settle rounds hold collectives: both ranks must agree on their number, whatever their own clocks say; after
    #  them the reset and the warm-up steps run again, so that the timed regions start from the same state as without them)
    rewarm = warmup if line["settle_steps"] else 0
    assert r0["steps"] == r1["steps"] == warmup + line["settle_steps"] + rewarm + repeats * steps + extra
    assert line["full"] is True and r0["profiled"] and r1["profiled"]
    assert r0["resets_at_step"] == r1["resets_at_step"] == ([0, warmup + line["settle_steps"]] if rewarm else [0])
    assert (line["settle_steps"] > 0) == (settle_ms > 0) and line["settle_steps"] % warmup == 0
    if gather_every == 1:
        assert line["gather_every_1"] is None
    else:
        assert line["gather_every_1"]["steps"] == min(steps, 300) and line["gather_every_1"]["value"] > 0
    # what rank 0 holds after the last gather really came from the two ranks (the stand-in engine stamps its rank)
    for terms in r0["gathered_term"]:
        assert terms == [1, 2]
    for rewards in r0["gathered_rewards"]:
        assert rewards[0] < 1000.0 <= rewards[1] < 2000.0


@pytest.mark.parametrize("scaling,envs", [("weak", 1024), ("strong", 8192)])
def test_eight_rank_bench_of_baseline_config_3_on_gloo(tmp_path, scaling, envs):
    """The command DESIGN.md section 6 names for BASELINE config 3 (highway-v0, 8192 envs x 101 vehicles over 8 GPUs), at the
    rank count it will meet: `--gpus 8 --workload v0_n100 --envs-per-gpu 1024` (weak: 1024 per rank) and `--scaling strong
    --envs-per-gpu 8192` (the same 8 x 1024 as a remainder-free split of a fixed total), eight ranks on gloo with the stand-in
    engine -- shard sizes, the packed gather of eight ranks' blocks into rank 0's buffer, the one JSON line (round-4 verdict item 7)."""
    steps, warmup, repeats, world = 5, 2, 2, 8
    argv = ["--gpus", str(world), "--workload", "v0_n100", "--steps", str(steps), "--warmup", str(warmup), "--repeats", str(repeats),
            "--envs-per-gpu", str(envs), "--scaling", scaling, "--gather-every", "4", "--settle-ms", "0", "--full", "--no-cpu-baseline"]
    res = _run(tmp_path, argv, world=world)
    assert all(r["lines"] == [] for r in res[1:]) and len(res[0]["lines"]) == 1
    line = res[0]["lines"][0]
    assert [r["envs"] for r in res] == [1024] * world                       # every rank steps its 1024-environment shard
    assert line["n_gpus"] == world and line["scaling"] == scaling and line["config"]["world_size_reported_by_the_process_group"] == world
    assert line["config"]["envs_per_gpu"] == 1024 and line["config"]["vehicles_per_env"] == 101
    assert line["value"] == pytest.approx(steps * 1024 * world / (line["ms_per_step"] * 1e-3 * steps), rel=1e-9)
    assert line["roofline"]["algorithmic_bytes_per_launch"] == 1024 * (72 * 101 + 110)   # 7,382 B per env-step
    assert len({r["steps"] for r in res}) == 1                              # the ranks agree on the number of steps (collectives)
    for terms in res[0]["gathered_term"]:
        assert terms == list(range(1, world + 1))                           # rank r's block landed in slot r of the root's buffer
    for rewards in res[0]["gathered_rewards"]:
        assert all(1000.0 * r <= rewards[r] < 1000.0 * (r + 1) for r in range(world))


# what only --full measures: the kernel-event region and the roofline view, the one-gather-per-step leg, K steps per launch, the
# host-pointer path, the Python front ends, the CPU leg, BASELINE's other workloads
FULL_ONLY = ("roofline", "gather_every_1", "rollout_k16", "host_path_env_steps_per_s", "frontend", "cpu_baseline", "secondary_workloads")


@pytest.mark.parametrize("world,gather_every", [(1, 1), (2, 4)])
def test_a_plain_run_times_the_headline_alone(tmp_path, world, gather_every):
    """Without --full a run sets up, warms up, settles, times its regions and prints the line -- nothing else steps the engine
    (the stand-in engine has no host-pointer step and no GPU behind it: any other leg would fail here)."""
    steps, warmup, repeats = 6, 3, 2
    argv = ["--gpus", str(world), "--steps", str(steps), "--warmup", str(warmup), "--repeats", str(repeats), "--envs-per-gpu", "4",
            "--gather-every", str(gather_every), "--settle-ms", "30"]
    res = _run(tmp_path, argv, world=world)
    assert len(res[0]["lines"]) == 1 and all(r["lines"] == [] for r in res[1:])
    line = res[0]["lines"][0]
    assert line["metric"] == line["unit"] == "env-steps/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["value"] == pytest.approx(4 * world / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert len(line["ms_per_step_repeats"]) == repeats and line["n_gpus"] == world
    assert line["full"] is False and not [k for k in FULL_ONLY if k in line], sorted(line)
    settle = line["settle_steps"]
    assert settle > 0 and settle % warmup == 0
    for r in res:  # warm-up, settling, the same reset and warm-up again, the timed regions
        assert r["steps"] == warmup + settle + warmup + repeats * steps and not r["profiled"]
        assert r["resets_at_step"] == [0, warmup + settle]


def test_split_batch_is_a_leg_of_full():
    sys.path.insert(0, ROOT)
    import bench
    with pytest.raises(SystemExit) as ex:
        bench.main(["--split-batch", "2"], platform=CpuPlatform(0), emit=lambda line: None)
    assert ex.value.code == 2   # (argparse's usage error, before anything touches a device)


def test_the_secondary_legs_of_a_full_run_are_full_runs(monkeypatch):
    """--full reports every secondary workload with its kernel duration and issue limits: each leg's own line must carry its
    roofline, so each leg runs with --full too."""
    import subprocess
    sys.path.insert(0, ROOT)
    import bench
    leg = {"ms_per_step": 0.2, "ms_per_step_device": 0.19, "value": 5e6, "unit": "env-steps/s", "vehicle_steps_per_s": 5e8,
           "roofline": {"avg_kernel_us": 180.0, "kernel": "k", "frac": 0.01, "algorithmic_bytes_per_launch": 7, "valu": None}}
    cmds = []

    def run(cmd, **kw):
        cmds.append(cmd)
        return subprocess.CompletedProcess(cmd, 0, stdout=json.dumps(leg) + "\n", stderr="")
    monkeypatch.setattr(subprocess, "run", run)
    out = bench.secondary_workloads()
    assert len(cmds) == len(bench.SECONDARY) and all("--full" in c for c in cmds)
    assert [v.get("avg_kernel_us") for v in out.values()] == [180.0] * len(bench.SECONDARY), out


def test_dump_outputs_writes_the_last_timed_step_of_every_rank(tmp_path):
    """--dump-outputs: after the timed regions, what the LAST timed step returned -- every rank's block, gathered to rank 0, in rank
    order -- as .npy files in float32 / float64 (the stand-in engine stamps its rank and its running step count)."""
    steps, warmup, repeats, envs = 6, 3, 2, 4
    out = tmp_path / "dump"
    argv = ["--gpus", "2", "--steps", str(steps), "--warmup", str(warmup), "--repeats", str(repeats), "--envs-per-gpu", str(envs),
            "--gather-every", "4", "--settle-ms", "30", "--no-cpu-baseline", "--dump-outputs", str(out)]
    r0, r1 = _run(tmp_path, argv)
    line = r0["lines"][0]
    settle = line["settle_steps"]
    assert settle > 0
    d = line["dumped_outputs"]
    assert d["step"] == warmup + repeats * steps - 1 and d["envs"] == d["envs_written"] == 2 * envs
    assert sorted(p.name for p in out.iterdir()) == sorted(k + ".npy" for k in d["files"])
    arr = {k: np.load(out / (k + ".npy")) for k in d["files"]}
    assert set(arr) == {"obs", "reward", "terminated", "truncated", "info_speed", "info_crashed"}
    assert arr["obs"].dtype == np.float32 and arr["obs"].shape == (2 * envs, 1, 5, 5)
    assert arr["reward"].dtype == np.float64 and arr["reward"].shape == (2 * envs, 1)
    assert arr["terminated"].dtype == np.float32 and arr["terminated"].shape == (2 * envs,)
    # the engine's step count at the last timed step: warm-up, settling, the repeated warm-up after it, the timed regions
    last = warmup + settle + warmup + repeats * steps
    np.testing.assert_array_equal(arr["reward"][:, 0], [last] * envs + [1000.0 + last] * envs)
    np.testing.assert_array_equal(arr["obs"][:, 0, 0, 0], [0.0] * envs + [1.0] * envs)
    np.testing.assert_array_equal(arr["terminated"], [1.0] * envs + [2.0] * envs)
    assert d["bytes"] == sum(a.nbytes for a in arr.values())


def test_dump_outputs_keeps_a_fixed_sample_past_the_size_limit(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    E, A = 50, 2
    rng = np.random.default_rng(3)

    def views(lo):
        return {"obs": torch.from_numpy(rng.standard_normal((E, A, 5, 5)).astype(np.float32)),
                "reward": torch.from_numpy(np.arange(lo, lo + E * A, dtype=np.float64).reshape(E, A)),
                "info_speed": torch.zeros((E, A), dtype=torch.float64), "terminated": torch.ones(E, dtype=torch.uint8),
                "truncated": torch.zeros(E, dtype=torch.uint8), "info_crashed": torch.zeros((E, A), dtype=torch.uint8)}
    per_rank = [views(0), views(E * A)]
    full = bench.dump_outputs(str(tmp_path / "full"), per_rank)
    assert full["envs_written"] == 2 * E and "env_index" not in full["files"]
    limit = 40 * (A * 25 * 4 + 2 * A * 8 + 2 * 4 + A * 4)   # room for 40 environments, less their indices
    a = bench.dump_outputs(str(tmp_path / "a"), per_rank, limit_bytes=limit)
    b = bench.dump_outputs(str(tmp_path / "b"), per_rank, limit_bytes=limit)
    assert 0 < a["envs_written"] < 40 and a == dict(b, dir=a["dir"]) and a["bytes"] <= limit
    idx = np.load(tmp_path / "a" / "env_index.npy")
    assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0)
    np.testing.assert_array_equal(idx, np.load(tmp_path / "b" / "env_index.npy"))
    for k in ("obs", "reward", "terminated"):
        np.testing.assert_array_equal(np.load(tmp_path / "a" / (k + ".npy")), np.load(tmp_path / "full" / (k + ".npy"))[idx.astype(int)])
