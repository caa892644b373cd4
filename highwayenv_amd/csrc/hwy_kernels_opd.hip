// hwy_kernels_opd.hip -- gfx950 translation unit of the optimistic planner's tree kernel (hwy_opd.h: hwy_opd_kernel, one wavefront
// per environment) and its launch function.  Its own translation unit so that every kernel of the other units keeps its code and
// its register allocation.
#include <hip/hip_runtime.h>

#include "hwy_opd.h"
#include "hwy_launch.h"

namespace hwy {

// A plain launch: the dispatch timestamps of hwy_profile_* belong to the step kernel.
hipError_t launch_opd(const OpdParams &op, hipStream_t stream) {
  if (op.E < 1 || op.n < 1 || op.X < 1 || op.x < 0 || op.x > op.X || op.M != 1 + op.X * op.n || op.M > HWY_OPD_MAX_NODES || !op.ret ||
      !op.disc || !op.upper0 || !op.done || !op.expanded_node || !op.reward || !op.terminated || !op.truncated || !op.gather_src ||
      !op.scatter_src || !op.root_src || !op.actions || !op.action)
    return hipErrorInvalidValue;
  if ((op.child_mask != nullptr) != (op.created != nullptr)) return hipErrorInvalidValue;
  if (op.created) hipLaunchKernelGGL(hwy_opd_masked_kernel<HWY_OPD_MAX_NODES>, dim3(op.E), dim3(64), 0, stream, op);
  else hipLaunchKernelGGL(hwy_opd_kernel<HWY_OPD_MAX_NODES>, dim3(op.E), dim3(64), 0, stream, op);
  return hipGetLastError();
}

}  // namespace hwy
