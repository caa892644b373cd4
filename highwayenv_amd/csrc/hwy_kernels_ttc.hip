// hwy_kernels_ttc.hip -- gfx950 translation unit of the time-to-collision grid / finite-MDP planner kernel (hwy_ttc.h:
// hwy_ttc_kernel, one wavefront per (environment, agent)) and its launch function.  Its own translation unit so that every kernel of
// the other units keeps its code and its register allocation.
#include <hip/hip_runtime.h>

#include "hwy_ttc.h"
#include "hwy_launch.h"

namespace hwy {

// the unit's rules (hwy_launch_units.h) with the HIP backend
hipError_t launch_ttc(const TtcParams &tp, bool plan, int rows, hipStream_t stream) {
  return select_ttc<HipBackend>(tp, plan, rows, stream);
}

}  // namespace hwy
