"""Register / LDS allocation of the direct-ego-control kernels (hwy_kernels_direct.hip), read from the code object's own metadata
like tests/test_traffic_kernel_resources.py (no GPU needed).

gfx950: 512 VGPRs per SIMD lane (allocation granule 8), 160 KB of LDS per CU, 4 SIMDs per CU."""
import pytest

from highwayenv_amd import build

LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def res():
    pytest.importorskip("msgpack")
    if build.is_stale():
        build.build_engine()
    return build.kernel_resources()


def waves_per_simd(vgpr: int) -> int:
    return min(8, 512 // (((vgpr + 7) // 8) * 8))


def test_every_direct_kernel_is_in_the_library(res):
    for nw in (1, 2, 3, 4):
        assert f"hwy::hwy_reset_direct_kernel<{nw}>" in res
        for wpe in (1, 2, 3, 4):
            assert f"hwy::hwy_step_direct_kernel<{nw}, {wpe}>" in res
            assert f"hwy::hwy_rollout_direct_kernel<{nw}, {wpe}>" in res
    for wpe in (1, 2, 3, 4):
        for full in ("false", "true"):
            assert f"hwy::hwy_step_wave_direct_kernel<{wpe}, {full}>" in res
            assert f"hwy::hwy_rollout_wave_direct_kernel<{wpe}, {full}>" in res


def test_direct_wave_kernels_four_waves_per_simd_no_vgpr_spills(res):
    """N <= 64 (the headline shape): every allocation variant of the one-wavefront direct-control kernels stays at or below 128
    VGPRs -- four wavefronts per SIMD -- without a spilled VGPR, and holds 16 one-wavefront workgroups per CU by LDS, like the 99 /
    113 VGPRs of the meta-action builds."""
    for wpe in (1, 2, 3, 4):
        for full in ("false", "true"):
            for kind in ("step", "rollout"):
                r = res[f"hwy::hwy_{kind}_wave_direct_kernel<{wpe}, {full}>"]
                print(kind, wpe, full, r)
                assert r["vgpr_spill"] == 0, (kind, wpe, full, r)
                assert r["vgpr"] <= 128 and waves_per_simd(r["vgpr"]) >= 4, (kind, wpe, full, r)
                assert 16 * r["lds"] <= LDS_PER_CU, (kind, wpe, full, r)
                assert r["sgpr"] <= 106


def test_direct_workgroup_kernels_allocation(res):
    """N > 64 (or tune_block_kernel = 1).  What the engine relies on (hwy_create picks the 4-wave build when the grid exceeds three
    resident wavefronts per SIMD, the 3-wave build otherwise) is the OCCUPANCY of each build: wpe wavefronts per SIMD by registers.
    The 3-wave builds have 168 VGPRs to live in and must not spill; a 4-wave build is squeezed into 128 and may spill, but less
    than one allocation granule (8 VGPRs) -- beyond that the build no longer "almost fits" and the 3-wave build is the better
    kernel.  LDS: one environment's image, ~8.6 KB per wavefront."""
    for nw in (1, 2, 3, 4):
        for wpe in (3, 4):
            for kind in ("step", "rollout"):
                r = res[f"hwy::hwy_{kind}_direct_kernel<{nw}, {wpe}>"]
                print(kind, nw, wpe, r)
                assert r["vgpr_spill"] == 0 if wpe == 3 else r["vgpr_spill"] < 8, (kind, nw, wpe, r)
                assert waves_per_simd(r["vgpr"]) >= wpe, (kind, nw, wpe, r)
                assert r["lds"] <= nw * 8800, (kind, nw, wpe, r)
                assert r["sgpr"] <= 106
