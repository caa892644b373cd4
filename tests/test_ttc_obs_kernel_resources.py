"""What the compiler allocated to the TimeToCollision observation kernel (csrc/hwy_collision_obs.h), read from the built library's
gfx950 code objects (build.kernel_resources(); no GPU): exactly one new kernel, one wavefront per workgroup, no scratch, no spill,
no more LDS than the source declares, and registers for eight wavefronts per SIMD.  Its name stays clear of the substrings and the
pattern by which the other resource and variant tests select THEIR kernels."""
import pytest

from highwayenv_amd import _abi, build
from tests.variants_util import SHAPE_KERNEL, STEP_OR_ROLLOUT

KERNEL = f"hwy::hwy_collision_obs_kernel<{9 * _abi.HWY_MAX_TTC_STEPS}>"
TAKEN = ("ttc", "mdp", "mask", "final", "respawn", "fork", "score", "shape")


@pytest.fixture(scope="module")
def res():
    build.build_engine()
    return build.kernel_resources()


def test_exactly_one_new_kernel(res):
    """The unit's code object holds this kernel and nothing else that no other unit holds: every other name in it (the re-spawn
    kernels every unit that includes hwy_launch.h emits) is found in another code object too."""
    assert [k for k in res if "collision_obs" in k] == [KERNEL]
    units = build.kernel_resources_by_unit()
    mine = [u for u in units if KERNEL in u]
    assert len(mine) == 1
    elsewhere = set().union(*(set(u) for u in units if u is not mine[0]))
    assert set(mine[0]) - elsewhere == {KERNEL}, sorted(set(mine[0]) - elsewhere)
    assert not any(s in KERNEL for s in TAKEN) and not STEP_OR_ROLLOUT.match(KERNEL) and not SHAPE_KERNEL.match(KERNEL)


def test_allocation(res):
    from tests.emu import emu, emu_ttc_obs  # noqa: F401  (registers the unit)
    k = res[KERNEL]
    assert k["workgroup"] == 64
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
    assert 0 < k["lds"] <= emu.lib("ttc_obs").emu_ttc_obs_lds_bytes() == 2304, k   # nine rows of 64 dwords
    assert k["vgpr"] <= 64, k                                                      # 512 / 64: eight wavefronts per SIMD
