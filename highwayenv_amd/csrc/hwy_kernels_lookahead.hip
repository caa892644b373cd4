// hwy_kernels_lookahead.hip -- gfx950 translation unit of the environment fork and the rollout scoring kernels (hwy_lookahead.h:
// hwy_fork_kernel, one workgroup per destination environment; hwy_score_kernel, one wavefront per environment group) and their
// launch functions.  Its own translation unit so that every kernel of the other units keeps its code and its register allocation.
#include <hip/hip_runtime.h>

#include "hwy_lookahead.h"
#include "hwy_launch.h"

namespace hwy {

// Plain launches: the dispatch timestamps of hwy_profile_* belong to the step kernel.
hipError_t launch_fork(const ForkParams &fp, hipStream_t stream) {
  if (fp.dst_envs < 1 || fp.src_envs < 1 || fp.branches < 1 || fp.pitch < 1 || fp.n_f64 < 0 || fp.n_f64 > HWY_FORK_MAX_F64_PLANES ||
      fp.n_i32 < 0 || fp.n_i32 > HWY_FORK_MAX_I32_PLANES || fp.A < 1 || 2 * fp.A > HWY_FORK_THREADS ||
      (!fp.src_env && (long long)fp.src_envs * fp.branches < fp.dst_envs))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(hwy_fork_kernel<HWY_FORK_THREADS>, dim3(fp.dst_envs), dim3(HWY_FORK_THREADS), 0, stream, fp);
  return hipGetLastError();
}

hipError_t launch_score(const ScoreParams &sp, hipStream_t stream) {
  if (sp.groups < 1 || sp.branches < 1 || sp.K < 1 || sp.A < 1 || sp.n_ids < 1 || sp.n_ids > HWY_SCORE_MAX_IDS || !sp.reward ||
      !sp.terminated || !sp.truncated)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(hwy_score_kernel<HWY_SCORE_MAX_IDS>, dim3(sp.groups), dim3(64), 0, stream, sp);
  return hipGetLastError();
}

}  // namespace hwy
