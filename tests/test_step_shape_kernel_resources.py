"""What the compiler allocated to the one-wavefront step kernel compiled for the registered configurations (csrc/hwy_wave.h:
hwy_shape_wave_kernel<FixedShape<...>, WPE>; csrc/hwy_kernels_shapes.hip), read from the built library's code object: no spilled
VGPR, registers for WPE wavefronts per SIMD, the generic kernel's LDS -- a shape kernel is launched in the generic kernel's place,
with its grid, block and dynamic LDS, and the engine's issue-priority turns count the GENERIC kernel's resident workgroups -- and
fewer SGPRs spilled to VGPR lanes than the generic kernel, which is what a shape is for.  Every shape kernel of the code object is
one the launch layer can reach (csrc/hwy_launch_family.h: launch_step_shape), in this unit alone."""
import pytest

from highwayenv_amd import build

# FixedShape<id, lanes, hwy_config.flags, frames per step>: FastShape3, FastShape4, V0Shape4 and their generic counterpart's FULL_SCAN
SHAPES = {"hwy::FixedShape<1, 3, 89, 5>": "false", "hwy::FixedShape<2, 4, 89, 5>": "false", "hwy::FixedShape<3, 4, 25, 15>": "true"}


@pytest.fixture(scope="module")
def res():
    pytest.importorskip("msgpack")
    if build.is_stale():
        build.build_engine()
    return build.kernel_resources()


def waves_per_simd(vgpr: int) -> int:
    return min(8, 512 // (((vgpr + 7) // 8) * 8))  # gfx950: 512 VGPRs per SIMD lane, allocation granule 8


def test_the_shape_kernels_are_the_ones_the_launch_layer_reaches(res):
    want = sorted(f"hwy::hwy_shape_wave_kernel<{s}, {wpe}>" for s in SHAPES for wpe in (1, 2, 3, 4))
    assert sorted(k for k in res if "shape" in k) == want


def test_the_shape_kernels_live_in_their_own_unit():
    """hwy_kernels.hip launches them through a function it only declares (hwy_launch.h: extern template): ONE code object of the
    library holds the shape kernels, and it holds no generic step kernel."""
    objects = build.gfx950_code_objects(open(build.LIB_PATH, "rb").read())
    holders = [co for co in objects if b"hwy_shape_wave_kernel" in co]
    assert len(holders) == 1 and b"hwy_step_wave_kernel" not in holders[0]


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("wpe", [1, 2, 3, 4])
def test_shape_kernel_allocation(res, shape, wpe):
    r = res[f"hwy::hwy_shape_wave_kernel<{shape}, {wpe}>"]
    g = res[f"hwy::hwy_step_wave_kernel<{wpe}, {SHAPES[shape]}>"]
    assert r["vgpr_spill"] == 0 and r["scratch"] <= 36, r  # (36 B: the frame next to SGPRs spilled to VGPR lanes, as in the generic kernel)
    assert waves_per_simd(r["vgpr"]) >= wpe and r["workgroup"] == 64, r
    assert r["lds"] == g["lds"], (r, g)
    # measured on this build, every WPE alike -- FastShape3 / FastShape4: 101 VGPRs (generic 99), 2 SGPRs spilled to VGPR lanes
    # (generic 83), no scratch frame (generic 36 B); V0Shape4: 115 VGPRs (generic 113), 4 spilled SGPRs (generic 85)
    assert r["vgpr"] <= (104 if SHAPES[shape] == "false" else 120), r  # (the allocation granule above the measured count)
    assert r["sgpr_spill"] <= 8 and r["sgpr_spill"] < g["sgpr_spill"], (r, g)
