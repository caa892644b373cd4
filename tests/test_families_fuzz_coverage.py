"""What the fuzz of the Linear, direct-control and Lidar families (tests/test_fuzz_configs.py) can compare in full, established on
the ORACLE ALONE: rollout()'s one exclusion is a collision whose push direction the oracle itself reports within 1e-6 of the knife
edge, so the share of live env-steps under it is a property of the draws, not of any kernel.  The fuzz asserts that every chunk
compares at least FULL_FLOOR of its live env-steps in full; this test holds the draw ranges to that on chunks 0..99, CPU only."""
import pytest

from tests.test_fuzz_configs import FULL_FLOOR, run_family_chunk


@pytest.mark.parametrize("family", ["linear", "direct", "lidar"])
def test_draws_leave_ninety_percent_comparable(family):
    worst, tot = 1.0, {"live": 0, "full": 0, "excluded": 0}
    for chunk in range(100):
        stats = run_family_chunk(family, chunk, None)
        assert stats["live"] > 0
        assert stats["full"] >= FULL_FLOOR * stats["live"], f"chunk {chunk}: {stats}"
        worst = min(worst, stats["full"] / stats["live"])
        for k in tot:
            tot[k] += stats[k]
    print(f"\n{family}: chunks 0..99, oracle alone: {tot}; least share compared in full in a chunk: {100 * worst:.1f} %")
