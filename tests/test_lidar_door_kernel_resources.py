"""What the compiler allocated to every instantiation of the Lidar door's kernel (csrc/hwy_lidar_door.h), read from the built
library's gfx950 code objects (build.kernel_resources(); no GPU): one 64-thread workgroup, no scratch, no spilled register, and LDS
that lets 16 workgroups share the 160 KB of a CU, as tests/test_lidar_kernel_resources.py demands of the configured kernel -- the
four cells per lane of the 256-cell instantiations live in registers, not in LDS.  The kernel's name stays clear of the pattern by
which the variant tests select the step kernels, and the configured kernel is still there under its own."""
import pytest

from highwayenv_amd import build
from tests.variants_util import SHAPE_KERNEL, STEP_OR_ROLLOUT

LDS_PER_CU = 160 * 1024
KERNELS = [f"hwy::hwy_lidar_any_kernel<{n}, {cpl}>" for n in ("true", "false") for cpl in (1, 4)]


@pytest.fixture(scope="module")
def res():
    pytest.importorskip("msgpack")
    if build.is_stale():
        build.build_engine()
    return build.kernel_resources()


def waves_per_simd(vgpr: int) -> int:
    return min(8, 512 // (((vgpr + 7) // 8) * 8))


def test_the_instantiations_and_their_names(res):
    assert sorted(k for k in res if "lidar_any" in k) == sorted(KERNELS)
    assert {"hwy::hwy_lidar_kernel<true>", "hwy::hwy_lidar_kernel<false>"} <= set(res)
    for k in KERNELS:
        assert not STEP_OR_ROLLOUT.match(k) and not SHAPE_KERNEL.match(k), k
    units = [u for u in build.kernel_resources_by_unit() if KERNELS[0] in u]
    assert len(units) == 1 and all(k in units[0] for k in KERNELS)  # one translation unit holds all four


@pytest.mark.parametrize("name", KERNELS)
def test_allocation(res, name):
    r = res[name]
    print(name, r)
    assert r["workgroup"] == 64
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, r
    assert 16 * r["lds"] <= LDS_PER_CU, r
    assert r["lds"] == 64 * (11 * 8 + 4), r        # phase 1's 92 bytes per obstacle of a 64-obstacle pass, whatever the cells per lane
    assert waves_per_simd(r["vgpr"]) >= 4, r       # four wavefronts per SIMD by registers: the 16 workgroups per CU of the LDS bound
