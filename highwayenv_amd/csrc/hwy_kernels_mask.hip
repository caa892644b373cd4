// hwy_kernels_mask.hip -- gfx950 translation unit of the action-mask kernel (hwy_mask.h: hwy_mask_kernel, one thread per
// (environment, agent)) and its launch function.  Its own translation unit so that every kernel of the other units keeps its code
// and its register allocation.
#include <hip/hip_runtime.h>

#include "hwy_mask.h"

namespace hwy {

// mp.rows (environment, agent) pairs, row r written to mp.mask + r * n_ids.  A plain launch: the dispatch timestamps of
// hwy_profile_* belong to the step kernel.
hipError_t launch_mask(const MaskParams &mp, hipStream_t stream) {
  if (mp.rows < 1 || mp.A < 1 || mp.N < 1 || mp.N > mp.pitch || mp.n_lanes < 0 || mp.n_lanes > HWY_MAX_LANES || !mp.x || !mp.y ||
      !mp.packed || !mp.mask || mp.n_ids != HWY_NUM_ACTIONS(mp.action_set))
    return hipErrorInvalidValue;
  const unsigned blocks = ((unsigned)mp.rows + HWY_MASK_BLOCK - 1) / HWY_MASK_BLOCK;
  hipLaunchKernelGGL(hwy_mask_kernel<HWY_MASK_BLOCK>, dim3(blocks), dim3(HWY_MASK_BLOCK), 0, stream, mp);
  return hipGetLastError();
}

}  // namespace hwy
