"""What the compiler allocated to the fork and scoring kernels (csrc/hwy_lookahead.h), read from the built library's code object:
no scratch, no spilled registers; the scoring kernel's LDS is its 256 per-action slots of 8 bytes plus two maxima and two indices;
the fork kernel uses no LDS; both leave eight wavefronts per SIMD their registers.  Their names are not step or rollout kernels
(tests/variants_util.py: STEP_OR_ROLLOUT is checked complete against the code object)."""
import pytest

from highwayenv_amd import build
from tests import variants_util

KERNELS = {"hwy::hwy_fork_kernel<256>": dict(lds=0, workgroup=256, vgpr=32),
           "hwy::hwy_score_kernel<256>": dict(lds=256 * 8 + 2 * 8 + 2 * 4, workgroup=64, vgpr=64)}


@pytest.fixture(scope="module")
def res():
    return build.kernel_resources()


def test_only_these_lookahead_kernels_exist(res):
    assert sorted(k for k in res if "fork" in k or "score" in k) == sorted(KERNELS)
    assert not any(variants_util.STEP_OR_ROLLOUT.match(k) for k in KERNELS)


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_lookahead_kernel_allocation(res, name):
    k, want = res[name], KERNELS[name]
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
    assert k["workgroup"] == want["workgroup"]
    assert k["lds"] <= want["lds"], k
    assert k["vgpr"] <= want["vgpr"], k   # 512 / 64: eight wavefronts per SIMD are not limited by registers
