// hwy_kernels_collision_obs.hip -- gfx950 translation unit of the TimeToCollision observation kernel (hwy_collision_obs.h:
// hwy_collision_obs_kernel, one wavefront per (environment, agent)) and its launch function.  Its own translation unit so that every
// kernel of the other units keeps its code and its register allocation.
#include <hip/hip_runtime.h>

#include "hwy_collision_obs.h"
#include "hwy_launch.h"

namespace hwy {

// the unit's rule (hwy_launch_units.h) with the HIP backend
hipError_t launch_collision_obs(const CollisionObsParams &cp, int rows, hipStream_t stream) {
  return select_collision_obs<HipBackend>(cp, rows, stream);
}

}  // namespace hwy
