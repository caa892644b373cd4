// hwy_kernels_ttc.hip -- gfx950 translation unit of the time-to-collision grid / finite-MDP planner kernel (hwy_ttc.h:
// hwy_ttc_kernel, one wavefront per (environment, agent)) and its launch function.  Its own translation unit so that every kernel of
// the other units keeps its code and its register allocation.
#include <hip/hip_runtime.h>

#include "hwy_ttc.h"
#include "hwy_launch.h"

namespace hwy {

// `rows` (environment, agent) pairs.  The grid lives in LDS at one dword per cell: two capacity classes, so that the common shapes
// (<= 1024 cells: 4 KB) keep many workgroups per CU and only the largest grids (up to 8 x 16 x 64 cells: 32 KB) pay for theirs.
// A plain launch: the dispatch timestamps of hwy_profile_* belong to the step kernel.
hipError_t launch_ttc(const TtcParams &tp, bool plan, int rows, hipStream_t stream) {
  const int cells = tp.V * tp.L * tp.T;
  if (rows < 1 || tp.V < 1 || tp.V > HWY_MAX_TARGET_SPEEDS || tp.L < 1 || tp.L > HWY_MAX_LANES || tp.T < 1 || tp.T > HWY_MAX_TTC_STEPS ||
      tp.N < 1 || tp.N > HWY_MAX_VEHICLES || (plan ? !tp.action : !tp.grid))
    return hipErrorInvalidValue;
  const bool small = cells <= HWY_TTC_SMALL_CELLS;
  if (plan) {
    if (small) hipLaunchKernelGGL((hwy_ttc_kernel<HWY_TTC_SMALL_CELLS, true>), dim3(rows), dim3(64), 0, stream, tp);
    else hipLaunchKernelGGL((hwy_ttc_kernel<HWY_TTC_MAX_CELLS, true>), dim3(rows), dim3(64), 0, stream, tp);
  } else {
    if (small) hipLaunchKernelGGL((hwy_ttc_kernel<HWY_TTC_SMALL_CELLS, false>), dim3(rows), dim3(64), 0, stream, tp);
    else hipLaunchKernelGGL((hwy_ttc_kernel<HWY_TTC_MAX_CELLS, false>), dim3(rows), dim3(64), 0, stream, tp);
  }
  return hipGetLastError();
}

}  // namespace hwy
