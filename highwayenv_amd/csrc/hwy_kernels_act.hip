// hwy_kernels_act.hip -- gfx950 translation unit of the continuous-action kernel (hwy_act.h: hwy_act_continuous_kernel, one thread
// per (environment, agent)) and its launch function.  Its own translation unit so that every kernel of the other units keeps its
// code and its register allocation.
#include <hip/hip_runtime.h>

#include "hwy_act.h"
#include "hwy_launch.h"

namespace hwy {

// the unit's rules (hwy_launch_units.h) with the HIP backend
hipError_t launch_act_continuous(const ActParams &ap, hipStream_t stream) {
  return select_act_continuous<HipBackend>(ap, stream);
}

}  // namespace hwy
