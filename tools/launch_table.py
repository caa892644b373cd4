#!/usr/bin/env python3
"""Developer tool: does a refactor of the host launch layer still launch the same kernels?  Needs an MI355X.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT_A -- python tools/launch_table.py     (HWY_ENGINE_LIB = library A)
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT_B -- python tools/launch_table.py     (HWY_ENGINE_LIB = library B)
    python tools/launch_table.py --compare OUT_A OUT_B                               exit status 0 = the same launches
    python tools/launch_table.py --covers OUT_A                                      exit status 0 = every step / rollout build ran

Without arguments: resets, steps, observes and runs a 2-step rollout once each on a table of tiny engines (4 environments) that
covers every branch of the kernel selection (csrc/hwy_launch_family.h, hwy_launch_rules.h): the one-wavefront kernel with and
without FULL_SCAN, the wide kernel, the workgroup kernel (OccupancyGrid, forced, N > 128), the Linear and direct families on both
sides of N = 64, the Lidar trace, the road-network kernels with both observations, the intersection kernel with and without helper
lanes, its 64-slot build and the doubled grid of next-episode pre-warming -- and then every row of tests/variants_util.py (the
branches in which hwy_config.tune_waves_per_eu picks a register-allocation build) at every value of the knob -- and then the
launches of the add-on units (csrc/hwy_launch_units.h): the TTC grid and plan on both sides of the 1024-cell LDS class, the Lidar
trace with and without normalisation, the fork with and without indices, the score of one and of several agents, an OPD plan of
budget 10 unmasked and masked, and the action mask on the highway, the merge and the intersection.  --compare reads the
two kernel traces in the order of the dispatch ids and requires equal sequences of (kernel name, grid size, workgroup size, LDS).  --covers reads
one trace and lists which step and rollout kernels of the built code object (highwayenv_amd.build.kernel_resources) were and were
not launched: the evidence that the selection rules as tests/variants_util.py restates them are what the engine really launches."""
from __future__ import annotations

import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINEAR = "highway_env.vehicle.behavior.LinearVehicle"


def table():
    """(label, config dict, make_config keywords, auto-reset)"""
    from highwayenv_amd import _abi, intersection, merge

    def hwy(n, **over):
        d = _abi.highway_default_config()
        d.update({"vehicles_count": n - 1, **over})
        return d

    def ix(slots, **over):
        d = intersection.intersection_default_config()
        d.update({"max_vehicles": slots, "host_traffic": False, **over})
        return d

    from tests import variants_util

    grid = {"observation": {"type": "OccupancyGrid"}}
    variants = [(f"{label} waves_per_eu={v}", d, variants_util.with_tuning(kw, waves_per_eu=v), False)
                for label, d, kw in variants_util.rows() for v in variants_util.values(kw)]
    return [
        ("N=50 ego-only collisions", hwy(50), {"fast": True}, False),
        ("N=50 full scan", hwy(50), {}, False),
        ("N=101 Kinematics", hwy(101), {}, False),
        ("N=101 OccupancyGrid", hwy(101, **grid), {}, False),
        ("N=101 block_kernel=1", hwy(101), {"tuning": {"block_kernel": 1}}, False),
        ("N=150 block_kernel=0", hwy(150), {}, False),
        ("N=150 block_kernel=2", hwy(150), {"tuning": {"block_kernel": 2}}, False),
        ("N=200 block_kernel=2", hwy(200), {"tuning": {"block_kernel": 2}}, False),
        ("Linear N=50", hwy(50, other_vehicles_type=LINEAR), {}, False),
        ("Linear N=101", hwy(101, other_vehicles_type=LINEAR), {}, False),
        ("Direct N=50", hwy(50, action={"type": "DiscreteAction"}), {}, False),
        ("Lidar N=50", hwy(50, observation={"type": "LidarObservation"}), {}, False),
        ("merge Kinematics", merge.merge_default_config(), {"scenario": "merge"}, False),
        ("merge OccupancyGrid", dict(merge.merge_default_config(), **grid), {"scenario": "merge"}, False),
        ("intersection N=30 helpers", ix(30), {"scenario": "intersection"}, False),
        ("intersection N=30 no helpers", ix(30), {"scenario": "intersection", "tuning": {"ix_no_helpers": 1}}, False),
        ("intersection N=40", ix(40), {"scenario": "intersection"}, False),
        ("intersection N=30 pre-warming", ix(30), {"scenario": "intersection"}, True),
    ] + variants


def run() -> None:
    import numpy as np

    from highwayenv_amd import _abi
    from highwayenv_amd.engine import Engine

    E = 4
    for label, d, kw, autoreset in table():
        cfg = _abi.make_config(d, E, **kw)
        eng = Engine(cfg)
        eng.reset(base_seed=11)
        if autoreset:
            eng.set_autoreset(True, base_seed=12)
        acts = np.ones((2, E, cfg.num_agents), np.int32)
        eng.step(acts[0])
        obs = eng.observe()
        out = eng.rollout(acts)
        eng.close()
        print(f"{label}: N={cfg.num_vehicles} obs {obs.shape} rollout {out[0].shape}", flush=True)


def run_units() -> None:
    """The add-on units' launches on 4-environment engines, every branch of csrc/hwy_launch_units.h."""
    import numpy as np

    from highwayenv_amd import _abi, intersection, merge
    from highwayenv_amd.engine import Engine

    E = 4

    def engine(d, num_envs=E, **kw):
        eng = Engine(_abi.make_config(d, num_envs, **kw))
        eng.reset(base_seed=11)
        return eng

    def hwy(**over):
        return dict(_abi.highway_fast_default_config(), vehicles_count=19, **over)

    # the TTC grid and the plan on it: 3 x 3 x 10 cells, and 3 x 6 x 64 = 1152 (the large LDS class)
    for d, horizon, tq in ((hwy(), 10.0, 1.0), (hwy(lanes_count=6), 6.4, 0.1)):
        eng, params = engine(d, fast=True), _abi.ttc_params(d, horizon=horizon, time_quantization=tq)
        grid = eng.ttc_grid(params)
        eng.mdp_plan(params, return_q=True, return_grid=True)
        eng.close()
        print(f"TTC {grid.shape[2:]}", flush=True)
    for normalize in (True, False):
        eng = engine(hwy(observation={"type": "LidarObservation", "normalize": normalize}), fast=True)
        print(f"Lidar normalize={normalize}: obs {eng.observe().shape}", flush=True)
        eng.close()
    # fork without and with indices; the score of a rollout of the branches, one agent and two
    for agents in (1, 2):
        d = hwy(controlled_vehicles=agents)
        src, dst = engine(d, fast=True), engine(d, 3 * E, fast=True)
        dst.fork_from(src, 3)
        dst.fork_from(src, 1, np.arange(3 * E, dtype=np.int32) % E)
        out = dst.score_rollout(np.ones((2, 3 * E, agents), np.int32), 3, 0.9)
        print(f"fork + score, {agents} agent(s): returns {out['returns'].shape}", flush=True)
        for e in (src, dst):
            e.close()
    for masked in (False, True):
        d = hwy(normalize_reward=True)
        src = engine(d, fast=True)
        params = _abi.opd_params(src.cfg, 10, 0.7, masked=masked)
        tree, work = engine(d, E * params.nodes, fast=True), engine(d, E * params.n_ids, fast=True)
        out = src.opd_plan(tree, work, params)
        print(f"opd_plan budget 10 masked={masked}: expanded {out['expanded'].tolist()}", flush=True)
        for e in (src, tree, work):
            e.close()
    ix = dict(intersection.intersection_default_config(), max_vehicles=30, host_traffic=False)
    for label, d, kw in (("highway", hwy(), {"fast": True}), ("merge", merge.merge_default_config(), {"scenario": "merge"}),
                         ("intersection", ix, {"scenario": "intersection"})):
        eng = engine(d, **kw)
        print(f"action mask {label}: {eng.action_mask().shape}", flush=True)
        eng.close()


def launches(out_dir: str) -> list:
    files = sorted(glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {out_dir}")
    rows = [r for f in files for r in csv.DictReader(open(f))]
    # in the order the host enqueued them: the three engines of an OPD plan have streams of their own, and two launches on different
    # streams (the root fork into `tree`, the parent fork into `work`) may START in either order
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))

    def cols(r, prefix):
        return tuple(int(r[k]) for k in sorted(r) if k.startswith(prefix))

    return [(r["Kernel_Name"], cols(r, "Grid_Size"), cols(r, "Workgroup_Size"), int(r["LDS_Block_Size"])) for r in rows]


def compare(a_dir: str, b_dir: str) -> int:
    a, b = launches(a_dir), launches(b_dir)
    print(f"{len(a)} launches in {a_dir}, {len(b)} in {b_dir}")
    diff = [(k, x, y) for k, (x, y) in enumerate(zip(a, b)) if x != y]
    for k, x, y in diff[:10]:
        print(f"launch {k}: {x} != {y}")
    same = len(a) == len(b) and not diff
    print(f"{len(set(x[0] for x in a))} distinct kernels;", "the two sequences are equal line for line" if same else "DIFFERENT")
    return 0 if same else 1


def covers(out_dir: str) -> int:
    import re

    from highwayenv_amd import build
    from tests.variants_util import STEP_OR_ROLLOUT

    # the trace names a kernel with its argument list ("void hwy::hwy_step_kernel<2, 4>(hwy::StepParams)"), kernel_resources() without
    ran = {re.sub(r"\(.*\)$", "", x[0]).replace("void ", "").strip() for x in launches(out_dir)}
    want = sorted(k for k in build.kernel_resources() if STEP_OR_ROLLOUT.match(k))
    missing = [k for k in want if k not in ran]
    print(f"{len(ran)} distinct kernels launched; {len(want) - len(missing)} of the {len(want)} step and rollout kernels of the code object among them")
    for k in want:
        print(("launched      " if k in ran else "NOT LAUNCHED  ") + k)
    print("not launched:", ", ".join(missing) if missing else "none")
    return 1 if missing else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) == 3 and sys.argv[1] == "--covers":
        sys.exit(covers(sys.argv[2]))
    run()
    run_units()
