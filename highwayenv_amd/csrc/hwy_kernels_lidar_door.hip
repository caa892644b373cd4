// hwy_kernels_lidar_door.hip -- gfx950 translation unit of the Lidar door's kernel (hwy_lidar_door.h: hwy_lidar_any_kernel, one
// wavefront per (environment, agent)) and its launch function.  Its own translation unit so that every kernel of the other units
// keeps its code and its register allocation.
#include <hip/hip_runtime.h>

#include "hwy_lidar_door.h"
#include "hwy_launch.h"

namespace hwy {

// the unit's rule (hwy_launch_units.h) with the HIP backend
hipError_t launch_lidar_door(const LidarDoorParams &lp, bool normalize, int rows, hipStream_t stream) {
  return select_lidar_door<HipBackend>(lp, normalize, rows, stream);
}

}  // namespace hwy
