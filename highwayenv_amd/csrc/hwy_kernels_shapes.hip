// hwy_kernels_shapes.hip -- gfx950 translation unit of the one-wavefront step kernel compiled for the registered shapes (hwy_wave.h:
// FixedShape, hwy_shape_wave_kernel): highway-fast-v0's structure on 3 and 4 lanes, highway-v0's on 4 lanes, each in the four
// register-allocation builds.  Which launch takes one: hwy_launch_family.h (step_shape_of); everything else launches the generic
// kernels of hwy_kernels.hip.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#define HWY_HAVE_SETPRIO 1  // (as in hwy_kernels.hip)
#include "hwy_device.h"
#include "hwy_wave.h"
#include "hwy_launch.h"

namespace hwy {
template hipError_t launch_step_shape<HipBackend>(int, const StepParams &, const Launch &);
}  // namespace hwy
