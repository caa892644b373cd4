// hwy_kernels_linear.hip -- gfx950 translation unit of the Linear traffic family (hwy_config.traffic_model == HWY_TRAFFIC_LINEAR):
// instantiates the LinearTraffic policy of the one-wavefront kernel (hwy_wave.h: hwy_step_wave_linear_kernel /
// hwy_rollout_wave_linear_kernel, N <= 64) and of the workgroup kernel (hwy_device.h: hwy_step_linear_kernel /
// hwy_rollout_linear_kernel / hwy_reset_linear_kernel) and their launch functions.  Its own translation unit because it is compiled
// without -amdgpu-sched-strategy=iterative-ilp (build.py: flags_for): the register allocator of ROCm 7.2's LLVM crashes on the
// workgroup kernel's Linear form under that scheduler.  The IDM kernels of hwy_kernels.hip keep their build.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#define HWY_HAVE_SETPRIO 1
#include "hwy_device.h"
#include "hwy_wave.h"
#include "hwy_launch.h"

namespace hwy {

void get_launch_events(hipEvent_t *start, hipEvent_t *stop);  // hwy_kernels.hip: the events of this thread's launches (hwy_profile_*)

static inline int waves_for(int n_vehicles) { return (n_vehicles + 63) / 64; }

template <typename K>
static hipError_t launch_lp(K kernel, int nw, int num_envs, hipStream_t stream, const LinearParams &lp, int lds = 0) {
  hipEvent_t start, stop;
  get_launch_events(&start, &stop);
  hipExtLaunchKernelGGL(kernel, dim3(num_envs), dim3(nw * 64), lds, stream, start, stop, 0, lp);
  return hipGetLastError();
}
// N <= 64: one wavefront per environment (FULL_SCAN = every vehicle checks collisions, highway-v0); lds = hwy_config.tune_extra_lds
template <int WPE>
static hipError_t launch_wave_linear_wpe(const LinearParams &lp, int num_envs, hipStream_t stream, int lds, bool rollout) {
  const bool fast = (lp.s.flags & HWY_C_EGO_ONLY_COLLISIONS) != 0;
  if (rollout) return fast ? launch_lp(hwy_rollout_wave_linear_kernel<WPE, false>, 1, num_envs, stream, lp, lds)
                           : launch_lp(hwy_rollout_wave_linear_kernel<WPE, true>, 1, num_envs, stream, lp, lds);
  return fast ? launch_lp(hwy_step_wave_linear_kernel<WPE, false>, 1, num_envs, stream, lp, lds)
              : launch_lp(hwy_step_wave_linear_kernel<WPE, true>, 1, num_envs, stream, lp, lds);
}
static hipError_t launch_wave_linear(const LinearParams &lp, int num_envs, hipStream_t stream, int waves_per_eu, int lds, bool rollout) {
  switch (waves_per_eu) {
    case 1: return launch_wave_linear_wpe<1>(lp, num_envs, stream, lds, rollout);
    case 2: return launch_wave_linear_wpe<2>(lp, num_envs, stream, lds, rollout);
    case 3: return launch_wave_linear_wpe<3>(lp, num_envs, stream, lds, rollout);
    default: return launch_wave_linear_wpe<4>(lp, num_envs, stream, lds, rollout);
  }
}
bool wave_linear_applies(const StepParams &p, bool force_block_kernel) { return p.N <= 64 && !force_block_kernel; }

// ceil(N / 64) wavefronts per environment, WPE = the register-allocation variant (hwy_engine.hip: waves_per_eu)
#define HWY_LINEAR_SWITCH(KERNEL, WPE)                                                          \
  switch (waves_for(lp.s.N)) {                                                                  \
    case 1: return launch_lp(KERNEL<1, WPE>, 1, num_envs, stream, lp);                          \
    case 2: return launch_lp(KERNEL<2, WPE>, 2, num_envs, stream, lp);                          \
    case 3: return launch_lp(KERNEL<3, WPE>, 3, num_envs, stream, lp);                          \
    case 4: return launch_lp(KERNEL<4, WPE>, 4, num_envs, stream, lp);                          \
    default: return hipErrorInvalidValue;                                                       \
  }
template <int WPE>
static hipError_t launch_step_linear_wpe(const LinearParams &lp, int num_envs, hipStream_t stream) { HWY_LINEAR_SWITCH(hwy_step_linear_kernel, WPE) }
template <int WPE>
static hipError_t launch_rollout_linear_wpe(const LinearParams &lp, int num_envs, hipStream_t stream) { HWY_LINEAR_SWITCH(hwy_rollout_linear_kernel, WPE) }
#undef HWY_LINEAR_SWITCH

hipError_t launch_step_linear(const LinearParams &lp, int num_envs, hipStream_t stream, int waves_per_eu, bool force_block_kernel,
                              int extra_lds) {
  if (wave_linear_applies(lp.s, force_block_kernel)) return launch_wave_linear(lp, num_envs, stream, waves_per_eu, extra_lds, false);
  switch (waves_per_eu) {
    case 1: return launch_step_linear_wpe<1>(lp, num_envs, stream);
    case 2: return launch_step_linear_wpe<2>(lp, num_envs, stream);
    case 3: return launch_step_linear_wpe<3>(lp, num_envs, stream);
    default: return launch_step_linear_wpe<4>(lp, num_envs, stream);
  }
}
hipError_t launch_rollout_linear(const LinearParams &lp, int num_envs, hipStream_t stream, int waves_per_eu, bool force_block_kernel,
                                 int extra_lds) {
  if (wave_linear_applies(lp.s, force_block_kernel)) return launch_wave_linear(lp, num_envs, stream, waves_per_eu, extra_lds, true);
  switch (waves_per_eu) {
    case 1: return launch_rollout_linear_wpe<1>(lp, num_envs, stream);
    case 2: return launch_rollout_linear_wpe<2>(lp, num_envs, stream);
    case 3: return launch_rollout_linear_wpe<3>(lp, num_envs, stream);
    default: return launch_rollout_linear_wpe<4>(lp, num_envs, stream);
  }
}
hipError_t launch_reset_linear(const LinearParams &lp, int num_envs, hipStream_t stream) {
  switch (waves_for(lp.s.N)) {
    case 1: return launch_lp(hwy_reset_linear_kernel<1>, 1, num_envs, stream, lp);
    case 2: return launch_lp(hwy_reset_linear_kernel<2>, 2, num_envs, stream, lp);
    case 3: return launch_lp(hwy_reset_linear_kernel<3>, 3, num_envs, stream, lp);
    case 4: return launch_lp(hwy_reset_linear_kernel<4>, 4, num_envs, stream, lp);
    default: return hipErrorInvalidValue;
  }
}

// workgroups of the Linear step kernel the device holds at once (issue-priority turns pay only when the whole grid is resident)
template <typename K>
static int resident(K kernel, int block, int lds = 0) {
  int per_cu = 0, dev = 0;
  hipDeviceProp_t prop;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, lds) != hipSuccess) return 0;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
  return per_cu * prop.multiProcessorCount;
}
template <int WPE>
static int resident_wpe(const StepParams &p, bool force_block_kernel, int lds) {
  if (wave_linear_applies(p, force_block_kernel))
    return (p.flags & HWY_C_EGO_ONLY_COLLISIONS) ? resident(hwy_step_wave_linear_kernel<WPE, false>, 64, lds)
                                                 : resident(hwy_step_wave_linear_kernel<WPE, true>, 64, lds);
  switch (waves_for(p.N)) {
    case 1: return resident(hwy_step_linear_kernel<1, WPE>, 64);
    case 2: return resident(hwy_step_linear_kernel<2, WPE>, 128);
    case 3: return resident(hwy_step_linear_kernel<3, WPE>, 192);
    case 4: return resident(hwy_step_linear_kernel<4, WPE>, 256);
    default: return 0;
  }
}
int step_linear_resident_blocks(const StepParams &p, int waves_per_eu, bool force_block_kernel, int extra_lds) {
  switch (waves_per_eu) {
    case 1: return resident_wpe<1>(p, force_block_kernel, extra_lds);
    case 2: return resident_wpe<2>(p, force_block_kernel, extra_lds);
    case 3: return resident_wpe<3>(p, force_block_kernel, extra_lds);
    default: return resident_wpe<4>(p, force_block_kernel, extra_lds);
  }
}

}  // namespace hwy
