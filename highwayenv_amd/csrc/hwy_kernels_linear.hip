// hwy_kernels_linear.hip -- gfx950 translation unit of the Linear traffic family (hwy_config.traffic_model == HWY_TRAFFIC_LINEAR):
// instantiates the LinearTraffic policy of the one-wavefront kernel (hwy_wave.h: hwy_step_wave_linear_kernel /
// hwy_rollout_wave_linear_kernel, N <= 64) and of the workgroup kernel (hwy_device.h: hwy_step_linear_kernel /
// hwy_rollout_linear_kernel / hwy_reset_linear_kernel); their selection is hwy_launch_family.h's (LinearFamily).  Its own translation unit
// because it is compiled without -amdgpu-sched-strategy=iterative-ilp (build.py: flags_for): the register allocator of ROCm 7.2's
// LLVM crashes on the workgroup kernel's Linear form under that scheduler.  The IDM kernels of hwy_kernels.hip keep their build.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#define HWY_HAVE_SETPRIO 1
#include "hwy_device.h"
#include "hwy_wave.h"
#include "hwy_launch.h"

namespace hwy {

hipError_t launch_step(const LinearParams &a, const Launch &l) { return select_step<HipBackend>(a, l, false); }
hipError_t launch_rollout(const LinearParams &a, const Launch &l) { return select_step<HipBackend>(a, l, true); }
hipError_t launch_reset(const LinearParams &a, const Launch &l) { return select_reset<HipBackend>(a, l); }
int step_resident_blocks(const LinearParams &a, const Launch &l) { return select_resident_blocks<HipBackend>(a, l); }

}  // namespace hwy
