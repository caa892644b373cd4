"""Register / LDS allocation of the LidarObservation kernel (hwy_kernels_lidar.hip), read from the code object's own metadata
like tests/test_control_kernel_resources.py (no GPU needed).

gfx950: 512 VGPRs per SIMD lane (allocation granule 8), 160 KB of LDS per CU, 4 SIMDs per CU."""
import pytest

from highwayenv_amd import build

LDS_PER_CU = 160 * 1024
KERNELS = ["hwy::hwy_lidar_kernel<true>", "hwy::hwy_lidar_kernel<false>"]


@pytest.fixture(scope="module")
def res():
    pytest.importorskip("msgpack")
    if build.is_stale():
        build.build_engine()
    return build.kernel_resources()


def waves_per_simd(vgpr: int) -> int:
    return min(8, 512 // (((vgpr + 7) // 8) * 8))


@pytest.mark.parametrize("name", KERNELS)
def test_lidar_kernel_allocation(res, name):
    """One 64-thread workgroup per (environment, agent): no spilled VGPR and no scratch, at least four wavefronts per SIMD by
    registers, and 16 workgroups per CU (four per SIMD) by LDS -- the 92 bytes per obstacle of a 64-obstacle pass."""
    assert name in res
    r = res[name]
    print(name, r)
    assert r["workgroup"] == 64
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, r
    assert waves_per_simd(r["vgpr"]) >= 4, r
    assert 16 * r["lds"] <= LDS_PER_CU, r
    assert r["lds"] == 64 * (11 * 8 + 4), r
