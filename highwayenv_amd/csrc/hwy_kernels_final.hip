// hwy_kernels_final.hip -- gfx950 translation unit of the SameStep stash (hwy_same_step.h: hwy_final_kernel, one workgroup per
// environment) and its launch function.  Its own translation unit so that every kernel of the other units keeps its code and its
// register allocation.
#include <hip/hip_runtime.h>

#include "hwy_same_step.h"
#include "hwy_launch.h"

namespace hwy {

// the unit's rules (hwy_launch_units.h) with the HIP backend
hipError_t launch_final(const FinalParams &fp, hipStream_t stream) {
  return select_final<HipBackend>(fp, stream);
}

}  // namespace hwy
