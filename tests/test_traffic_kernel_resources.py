"""Register / LDS allocation of the Linear traffic family's kernels (hwy_kernels_linear.hip), read from the code object's own
metadata like tests/test_kernel_resources.py (no GPU needed).  That translation unit is the library's SECOND gfx950 code object
(hwy_kernels.hip's is the first): build.kernel_resources reads every one.

gfx950: 512 VGPRs per SIMD lane (allocation granule 8), 160 KB of LDS per CU, 4 SIMDs per CU."""
import pytest

from highwayenv_amd import build

LDS_PER_CU = 160 * 1024

# The IDM kernels' allocation before the Linear family was added (vgpr, sgpr, vgpr_spill, sgpr_spill, lds): the family is compiled
# in its own translation unit and the shared templates take it as a compile-time policy, so none of these may move.
# (Two scalar-spill counts are those of the build whose reset and wide kernels call block_begin_episode / wide_begin_episode --
# hwy_reset_kernel<1> 42 -> 44, hwy_step_wide_kernel<3, 1> 207 -> 206, profiles/episode_start_refactor.md; every other figure is
# the one recorded then.)
IDM = {
    "hwy::hwy_observe_kernel<1>": (77, 106, 0, 42, 8512),
    "hwy::hwy_observe_kernel<2>": (83, 106, 0, 46, 17016),
    "hwy::hwy_observe_kernel<3>": (85, 106, 0, 48, 25520),
    "hwy::hwy_observe_kernel<4>": (87, 106, 0, 46, 34024),
    "hwy::hwy_reset_kernel<1>": (79, 106, 0, 44, 8512),
    "hwy::hwy_reset_kernel<2>": (85, 106, 0, 40, 17016),
    "hwy::hwy_reset_kernel<3>": (87, 106, 0, 40, 25520),
    "hwy::hwy_reset_kernel<4>": (89, 106, 0, 40, 34024),
    "hwy::hwy_rollout_kernel<1, 1>": (115, 106, 0, 44, 8768),
    "hwy::hwy_rollout_kernel<1, 2>": (115, 106, 0, 44, 8768),
    "hwy::hwy_rollout_kernel<1, 3>": (115, 106, 0, 44, 8768),
    "hwy::hwy_rollout_kernel<1, 4>": (115, 106, 0, 44, 8768),
    "hwy::hwy_rollout_kernel<2, 1>": (123, 106, 0, 45, 17280),
    "hwy::hwy_rollout_kernel<2, 2>": (123, 106, 0, 45, 17280),
    "hwy::hwy_rollout_kernel<2, 3>": (123, 106, 0, 45, 17280),
    "hwy::hwy_rollout_kernel<2, 4>": (123, 106, 0, 45, 17280),
    "hwy::hwy_rollout_kernel<3, 1>": (123, 106, 0, 45, 25776),
    "hwy::hwy_rollout_kernel<3, 2>": (123, 106, 0, 45, 25776),
    "hwy::hwy_rollout_kernel<3, 3>": (123, 106, 0, 45, 25776),
    "hwy::hwy_rollout_kernel<3, 4>": (123, 106, 0, 45, 25776),
    "hwy::hwy_rollout_kernel<4, 1>": (123, 106, 0, 45, 34288),
    "hwy::hwy_rollout_kernel<4, 2>": (123, 106, 0, 45, 34288),
    "hwy::hwy_rollout_kernel<4, 3>": (123, 106, 0, 45, 34288),
    "hwy::hwy_rollout_kernel<4, 4>": (123, 106, 0, 45, 34288),
    "hwy::hwy_rollout_wave_kernel<1, false>": (99, 106, 0, 46, 8080),
    "hwy::hwy_rollout_wave_kernel<1, true>": (113, 106, 0, 47, 8080),
    "hwy::hwy_rollout_wave_kernel<2, false>": (99, 106, 0, 46, 8080),
    "hwy::hwy_rollout_wave_kernel<2, true>": (113, 106, 0, 47, 8080),
    "hwy::hwy_rollout_wave_kernel<3, false>": (99, 106, 0, 46, 8080),
    "hwy::hwy_rollout_wave_kernel<3, true>": (113, 106, 0, 47, 8080),
    "hwy::hwy_rollout_wave_kernel<4, false>": (99, 106, 0, 46, 8080),
    "hwy::hwy_rollout_wave_kernel<4, true>": (113, 106, 0, 47, 8080),
    "hwy::hwy_step_kernel<1, 1>": (128, 106, 0, 137, 8768),
    "hwy::hwy_step_kernel<1, 2>": (128, 106, 0, 137, 8768),
    "hwy::hwy_step_kernel<1, 3>": (128, 106, 0, 137, 8768),
    "hwy::hwy_step_kernel<1, 4>": (128, 106, 0, 137, 8768),
    "hwy::hwy_step_kernel<2, 1>": (130, 106, 0, 139, 17280),
    "hwy::hwy_step_kernel<2, 2>": (130, 106, 0, 139, 17280),
    "hwy::hwy_step_kernel<2, 3>": (130, 106, 0, 139, 17280),
    "hwy::hwy_step_kernel<2, 4>": (128, 106, 2, 139, 17280),
    "hwy::hwy_step_kernel<3, 1>": (130, 106, 0, 143, 25776),
    "hwy::hwy_step_kernel<3, 2>": (130, 106, 0, 143, 25776),
    "hwy::hwy_step_kernel<3, 3>": (130, 106, 0, 143, 25776),
    "hwy::hwy_step_kernel<3, 4>": (128, 106, 2, 143, 25776),
    "hwy::hwy_step_kernel<4, 1>": (130, 106, 0, 139, 34288),
    "hwy::hwy_step_kernel<4, 2>": (130, 106, 0, 139, 34288),
    "hwy::hwy_step_kernel<4, 3>": (130, 106, 0, 139, 34288),
    "hwy::hwy_step_kernel<4, 4>": (128, 106, 2, 139, 34288),
    "hwy::hwy_step_wave_kernel<1, false>": (99, 106, 0, 83, 8080),
    "hwy::hwy_step_wave_kernel<1, true>": (113, 106, 0, 85, 8080),
    "hwy::hwy_step_wave_kernel<2, false>": (99, 106, 0, 83, 8080),
    "hwy::hwy_step_wave_kernel<2, true>": (113, 106, 0, 85, 8080),
    "hwy::hwy_step_wave_kernel<3, false>": (99, 106, 0, 83, 8080),
    "hwy::hwy_step_wave_kernel<3, true>": (113, 106, 0, 85, 8080),
    "hwy::hwy_step_wave_kernel<4, false>": (99, 106, 0, 83, 8080),
    "hwy::hwy_step_wave_kernel<4, true>": (113, 106, 0, 85, 8080),
    "hwy::hwy_step_wide_kernel<2, 2>": (235, 106, 0, 110, 15656),
    "hwy::hwy_step_wide_kernel<3, 1>": (318, 104, 0, 206, 22968),
    "hwy::hwy_step_wide_kernel<4, 1>": (430, 106, 0, 328, 30280),
}


@pytest.fixture(scope="module")
def res():
    pytest.importorskip("msgpack")
    if build.is_stale():
        build.build_engine()
    return build.kernel_resources()


def waves_per_simd(vgpr: int) -> int:
    return min(8, 512 // (((vgpr + 7) // 8) * 8))


def test_every_linear_kernel_is_in_the_library(res):
    for nw in (1, 2, 3, 4):
        assert f"hwy::hwy_reset_linear_kernel<{nw}>" in res
        for wpe in (1, 2, 3, 4):
            assert f"hwy::hwy_step_linear_kernel<{nw}, {wpe}>" in res
            assert f"hwy::hwy_rollout_linear_kernel<{nw}, {wpe}>" in res
    for wpe in (1, 2, 3, 4):
        for full in ("false", "true"):
            assert f"hwy::hwy_step_wave_linear_kernel<{wpe}, {full}>" in res
            assert f"hwy::hwy_rollout_wave_linear_kernel<{wpe}, {full}>" in res


def test_linear_wave_kernels_four_waves_per_simd_no_vgpr_spills(res):
    """N <= 64 (the headline shape): every allocation variant of the one-wavefront Linear kernels holds at least four wavefronts
    per SIMD by registers and 16 one-wavefront workgroups per CU by LDS, without a spilled VGPR -- like the IDM ones."""
    for wpe in (1, 2, 3, 4):
        for full in ("false", "true"):
            for kind in ("step", "rollout"):
                r = res[f"hwy::hwy_{kind}_wave_linear_kernel<{wpe}, {full}>"]
                assert r["vgpr_spill"] == 0, (kind, wpe, full, r)
                assert waves_per_simd(r["vgpr"]) >= 4, (kind, wpe, full, r)
                assert 16 * r["lds"] <= LDS_PER_CU, (kind, wpe, full, r)
                assert r["sgpr"] <= 106


def test_linear_workgroup_kernels_allocation(res):
    """N > 64 (or tune_block_kernel = 1): the 3-wave builds hold no spilled VGPR (130 / 131 VGPRs); the 4-wave builds, which the
    engine picks when the grid exceeds three resident wavefronts per SIMD (hwy_create), spill 2 VGPRs -- as the IDM workgroup kernel
    does from two wavefronts per environment on (IDM table below) -- and stay at four wavefronts per SIMD.  LDS: one environment's
    image, ~8.6 KB per wavefront."""
    for nw in (1, 2, 3, 4):
        for wpe in (3, 4):
            for kind in ("step", "rollout"):
                r = res[f"hwy::hwy_{kind}_linear_kernel<{nw}, {wpe}>"]
                assert r["vgpr_spill"] <= (0 if wpe == 3 else 2), (kind, nw, wpe, r)
                assert waves_per_simd(r["vgpr"]) >= wpe, (kind, nw, wpe, r)
                assert r["lds"] <= nw * 8800, (kind, nw, wpe, r)
                assert r["sgpr"] <= 106


def test_idm_kernels_are_untouched(res):
    for name, (vgpr, sgpr, vgpr_spill, sgpr_spill, lds) in IDM.items():
        r = res[name]
        assert (r["vgpr"], r["sgpr"], r["vgpr_spill"], r["sgpr_spill"], r["lds"]) == (vgpr, sgpr, vgpr_spill, sgpr_spill, lds), name
