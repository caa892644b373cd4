"""What the compiler allocated to the SameStep kernels (csrc/hwy_same_step.h: the stash; hwy_device.h, hwy_wave.h, hwy_wave2.h,
hwy_net.h: the re-spawn kernels), read from the built library's code object: they are there, none spills a vector register, the
stash uses no scratch, LDS or spill at all, and no name is one the variants table would take for a step, rollout or shape kernel
(tests/test_kernel_variants.py rejects a step or rollout kernel the table does not launch)."""
import pytest

from highwayenv_amd import build
from tests import variants_util

STASH = ["hwy::hwy_final_kernel<256>", "hwy::hwy_final_kernel<64>"]
RESPAWN = sorted(
    [f"hwy::hwy_respawn{family}_kernel<{nw}>" for family in ("", "_linear", "_direct") for nw in (1, 2, 3, 4)]
    + [f"hwy::hwy_respawn_wave{family}_kernel<1>" for family in ("", "_linear", "_direct")]
    + ["hwy::hwy_respawn_wide_kernel<2, 2>", "hwy::hwy_respawn_wide_kernel<3, 1>", "hwy::hwy_respawn_wide_kernel<4, 1>",
       "hwy::hwy_net_respawn_kernel<1, false>", "hwy::hwy_net_respawn_kernel<1, true>"])


@pytest.fixture(scope="module")
def res():
    return build.kernel_resources()


def test_only_these_same_step_kernels_exist(res):
    assert sorted(k for k in res if "respawn" in k) == RESPAWN
    assert sorted(k for k in res if "final" in k) == STASH
    for name in STASH + RESPAWN:
        assert not variants_util.STEP_OR_ROLLOUT.search(name) and not variants_util.SHAPE_KERNEL.search(name), name


def test_stash_allocation(res):
    for name, block in zip(STASH, (256, 64)):
        k = res[name]
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["lds"] == 0, (name, k)
        assert k["workgroup"] == block and k["vgpr"] <= 32, (name, k)


def test_respawn_kernels_spill_no_vector_register(res):
    """Like the reset kernels beside them they take the whole StepParams block by value, and the scalar registers that do not fit are
    kept in lanes of a vector register (sgpr_spill; the reset kernels: 40 .. 68) -- never in memory: no vector register is spilled."""
    for name in RESPAWN:
        k = res[name]
        assert k["vgpr_spill"] == 0, (name, k)
        assert k["sgpr_spill"] <= 68, (name, k)
        assert k["lds"] <= 64 * 1024, (name, k)
    for name in RESPAWN:
        if "wave" in name or "wide" in name or "net" in name:
            assert res[name]["workgroup"] == 64, name
