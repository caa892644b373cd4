// hwy_kernels_direct.hip -- gfx950 translation unit of direct ego control (hwy_config.ego_control == HWY_EGO_DIRECT, the
// reference's DiscreteAction): instantiates the DirectEgo policy of the one-wavefront kernel (hwy_wave.h: hwy_step_wave_direct_kernel
// / hwy_rollout_wave_direct_kernel, N <= 64) and of the workgroup kernel (hwy_device.h: hwy_step_direct_kernel /
// hwy_rollout_direct_kernel / hwy_reset_direct_kernel) with IDM traffic; their selection is hwy_launch_family.h's (DirectFamily).  Its own
// translation unit so that every kernel of hwy_kernels.hip and hwy_kernels_linear.hip keeps its code and its register allocation.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#define HWY_HAVE_SETPRIO 1
#include "hwy_device.h"
#include "hwy_wave.h"
#include "hwy_launch.h"

namespace hwy {

hipError_t launch_step(const DirectParams &a, const Launch &l) { return select_step<HipBackend>(a, l, false); }
hipError_t launch_rollout(const DirectParams &a, const Launch &l) { return select_step<HipBackend>(a, l, true); }
hipError_t launch_reset(const DirectParams &a, const Launch &l) { return select_reset<HipBackend>(a, l); }
int step_resident_blocks(const DirectParams &a, const Launch &l) { return select_resident_blocks<HipBackend>(a, l); }

}  // namespace hwy
