// hwy_kernels_opd.hip -- gfx950 translation unit of the optimistic planner's tree kernel (hwy_opd.h: hwy_opd_kernel, one wavefront
// per environment) and its launch function.  Its own translation unit so that every kernel of the other units keeps its code and
// its register allocation.
#include <hip/hip_runtime.h>

#include "hwy_opd.h"
#include "hwy_launch.h"

namespace hwy {

// the unit's rules (hwy_launch_units.h) with the HIP backend
hipError_t launch_opd(const OpdParams &op, hipStream_t stream) {
  return select_opd<HipBackend>(op, stream);
}

}  // namespace hwy
