"""Record the reference's RoadNetwork.shortest_path on the intersection-v0 network (tests/test_routes.py compares the host
planner of highwayenv_amd/intersection.py with it).

TEST INFRASTRUCTURE.  Needs the reference package (``HWY_REFERENCE_ROOT``, imported through ``oracle/ref_stub.py``):

    python tests/golden/make_golden_routes.py

Writes tests/golden/intersection_shortest_paths.json: for every node of the network and every exit "o0" .. "o3", the node list
the reference plans (an empty list where it finds no route)."""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_stub  # noqa: E402

OUT = os.path.join(HERE, "intersection_shortest_paths.json")


def shortest_paths() -> dict:
    ref_stub.install()
    from highway_env.envs.intersection_env import IntersectionEnv
    env = IntersectionEnv()
    env.reset(seed=0)
    net = env.road.network
    nodes = sorted(set(net.graph) | {b for a in net.graph for b in net.graph[a]})
    return {t: {f"o{k}": list(net.shortest_path(t, f"o{k}") or []) for k in range(4)} for t in nodes}


def main() -> None:
    if not ref_stub.reference_available():
        raise SystemExit(f"the reference package is not at {ref_stub.REFERENCE_ROOT} (set HWY_REFERENCE_ROOT)")
    paths = shortest_paths()
    with open(OUT, "w") as f:
        json.dump(paths, f, indent=1, sort_keys=True)
        f.write("\n")
    from tests.golden_util import record_fixture
    record_fixture("intersection_shortest_paths", os.path.basename(OUT), ["tests/golden/make_golden_routes.py"])
    print("wrote", OUT)


if __name__ == "__main__":
    main()
