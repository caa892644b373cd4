// hwy_kernels_lidar.hip -- gfx950 translation unit of the LidarObservation kernel (hwy_lidar.h: hwy_lidar_kernel, one wavefront per
// (environment, agent)) and its launch function.  Its own translation unit so that every kernel of hwy_kernels.hip,
// hwy_kernels_linear.hip and hwy_kernels_direct.hip keeps its code and its register allocation.
#include <hip/hip_runtime.h>

#include "hwy_lidar.h"
#include "hwy_launch.h"

namespace hwy {

// the unit's rules (hwy_launch_units.h) with the HIP backend
hipError_t launch_lidar(const LidarParams &lp, bool normalize, int rows, hipStream_t stream) {
  return select_lidar<HipBackend>(lp, normalize, rows, stream);
}

}  // namespace hwy
