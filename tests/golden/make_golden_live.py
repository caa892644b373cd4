"""Record the reference's traces of the random configurations of tests/test_oracle_live_reference.py.

TEST INFRASTRUCTURE.  Needs the reference package (``HWY_REFERENCE_ROOT``, imported through ``oracle/ref_stub.py``):

    python tests/golden/make_golden_live.py [live_highway_3 ...]

Cases 0 .. RECORDED_CASES - 1 of every family (highway / merge / intersection) are drawn exactly as the test draws them, run
through the fixture generators' run_scenario, and written to tests/golden/live/<name>.npz next to the scenario they were drawn
as (``scenario_json``).  A merge case whose rejection-sampled spawn places fewer traffic vehicles than there are agents to make
of them is recorded as ``skipped``, the reason the live run skips it with."""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_stub  # noqa: E402
from tests import test_oracle_live_reference as live  # noqa: E402
from tests.golden_util import record_fixture  # noqa: E402

OUT = os.path.join(HERE, "live")
SCENARIOS = [dict(live.SCENARIOS[family](case), family=family)
             for family in ("highway", "merge", "intersection") for case in range(live.RECORDED_CASES)]


def run_scenario(sc: dict) -> dict:
    """The file's arrays for one scenario of SCENARIOS."""
    family = sc["family"]
    sc = {k: v for k, v in sc.items() if k != "family"}
    out = {"scenario_json": np.asarray(live.scenario_json(sc))}
    try:
        data = live.run_live(family, sc)
    except IndexError:
        if family != "merge":
            raise
        return dict(out, skipped=np.asarray("fewer traffic vehicles than controlled_vehicles - 1"))
    return dict(out, **{k: np.asarray(v) for k, v in data.items()})


def main() -> None:
    if not ref_stub.reference_available():
        raise SystemExit(f"the reference package is not at {ref_stub.REFERENCE_ROOT} (set HWY_REFERENCE_ROOT)")
    only = set(sys.argv[1:])
    os.makedirs(OUT, exist_ok=True)
    for sc in SCENARIOS:
        if only and sc["name"] not in only:
            continue
        data = run_scenario(sc)
        path = os.path.join(OUT, sc["name"] + ".npz")
        np.savez_compressed(path, **data)
        record_fixture(sc["name"], "live/" + sc["name"] + ".npz",
                       ["tests/golden/make_golden_live.py", "tests/golden/" + live.GENERATORS[sc["family"]]])
        print(f"{sc['name']}: {'skipped' if 'skipped' in data else 'meta=' + str(data['meta'].tolist())} "
              f"-> {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
