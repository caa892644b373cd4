// hwy_kernels_lidar.hip -- gfx950 translation unit of the LidarObservation kernel (hwy_lidar.h: hwy_lidar_kernel, one wavefront per
// (environment, agent)) and its launch function.  Its own translation unit so that every kernel of hwy_kernels.hip,
// hwy_kernels_linear.hip and hwy_kernels_direct.hip keeps its code and its register allocation.
#include <hip/hip_runtime.h>

#include "hwy_lidar.h"
#include "hwy_launch.h"

namespace hwy {

// `rows` (environment, agent) pairs, row r written to lp.obs + r * cells * 2.  A plain launch: the dispatch timestamps of
// hwy_profile_* belong to the step kernel.
hipError_t launch_lidar(const LidarParams &lp, bool normalize, int rows, hipStream_t stream) {
  if (rows < 1 || lp.cells < 1 || lp.cells > HWY_MAX_LIDAR_CELLS) return hipErrorInvalidValue;
  if (normalize) hipLaunchKernelGGL(hwy_lidar_kernel<true>, dim3(rows), dim3(64), 0, stream, lp);
  else hipLaunchKernelGGL(hwy_lidar_kernel<false>, dim3(rows), dim3(64), 0, stream, lp);
  return hipGetLastError();
}

}  // namespace hwy
