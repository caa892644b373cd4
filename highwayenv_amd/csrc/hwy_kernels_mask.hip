// hwy_kernels_mask.hip -- gfx950 translation unit of the action-mask kernel (hwy_mask.h: hwy_mask_kernel, one thread per
// (environment, agent)) and its launch function.  Its own translation unit so that every kernel of the other units keeps its code
// and its register allocation.
#include <hip/hip_runtime.h>

#include "hwy_mask.h"
#include "hwy_launch.h"

namespace hwy {

// the unit's rules (hwy_launch_units.h) with the HIP backend
hipError_t launch_mask(const MaskParams &mp, hipStream_t stream) {
  return select_mask<HipBackend>(mp, stream);
}

}  // namespace hwy
