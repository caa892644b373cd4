// hwy_kernels_direct.hip -- gfx950 translation unit of direct ego control (hwy_config.ego_control == HWY_EGO_DIRECT, the
// reference's DiscreteAction): instantiates the DirectEgo policy of the one-wavefront kernel (hwy_wave.h: hwy_step_wave_direct_kernel
// / hwy_rollout_wave_direct_kernel, N <= 64) and of the workgroup kernel (hwy_device.h: hwy_step_direct_kernel /
// hwy_rollout_direct_kernel / hwy_reset_direct_kernel) with IDM traffic, and their launch functions.  Its own translation unit so
// that every kernel of hwy_kernels.hip and hwy_kernels_linear.hip keeps its code and its register allocation.
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
static hipError_t launch_dp(K kernel, int nw, int num_envs, hipStream_t stream, const DirectParams &dp, int lds = 0) {
  hipEvent_t start, stop;
  get_launch_events(&start, &stop);
  hipExtLaunchKernelGGL(kernel, dim3(num_envs), dim3(nw * 64), lds, stream, start, stop, 0, dp);
  return hipGetLastError();
}
// N <= 64: one wavefront per environment (FULL_SCAN = every vehicle checks collisions, highway-v0); lds = hwy_config.tune_extra_lds
template <int WPE>
static hipError_t launch_wave_direct_wpe(const DirectParams &dp, int num_envs, hipStream_t stream, int lds, bool rollout) {
  const bool fast = (dp.s.flags & HWY_C_EGO_ONLY_COLLISIONS) != 0;
  if (rollout) return fast ? launch_dp(hwy_rollout_wave_direct_kernel<WPE, false>, 1, num_envs, stream, dp, lds)
                           : launch_dp(hwy_rollout_wave_direct_kernel<WPE, true>, 1, num_envs, stream, dp, lds);
  return fast ? launch_dp(hwy_step_wave_direct_kernel<WPE, false>, 1, num_envs, stream, dp, lds)
              : launch_dp(hwy_step_wave_direct_kernel<WPE, true>, 1, num_envs, stream, dp, lds);
}
static hipError_t launch_wave_direct(const DirectParams &dp, int num_envs, hipStream_t stream, int waves_per_eu, int lds, bool rollout) {
  switch (waves_per_eu) {
    case 1: return launch_wave_direct_wpe<1>(dp, num_envs, stream, lds, rollout);
    case 2: return launch_wave_direct_wpe<2>(dp, num_envs, stream, lds, rollout);
    case 3: return launch_wave_direct_wpe<3>(dp, num_envs, stream, lds, rollout);
    default: return launch_wave_direct_wpe<4>(dp, num_envs, stream, lds, rollout);
  }
}
bool wave_direct_applies(const StepParams &p, bool force_block_kernel) { return p.N <= 64 && !force_block_kernel; }

// ceil(N / 64) wavefronts per environment, WPE = the register-allocation variant (hwy_engine.hip: waves_per_eu)
#define HWY_DIRECT_SWITCH(KERNEL, WPE)                                                          \
  switch (waves_for(dp.s.N)) {                                                                  \
    case 1: return launch_dp(KERNEL<1, WPE>, 1, num_envs, stream, dp);                          \
    case 2: return launch_dp(KERNEL<2, WPE>, 2, num_envs, stream, dp);                          \
    case 3: return launch_dp(KERNEL<3, WPE>, 3, num_envs, stream, dp);                          \
    case 4: return launch_dp(KERNEL<4, WPE>, 4, num_envs, stream, dp);                          \
    default: return hipErrorInvalidValue;                                                       \
  }
template <int WPE>
static hipError_t launch_step_direct_wpe(const DirectParams &dp, int num_envs, hipStream_t stream) { HWY_DIRECT_SWITCH(hwy_step_direct_kernel, WPE) }
template <int WPE>
static hipError_t launch_rollout_direct_wpe(const DirectParams &dp, int num_envs, hipStream_t stream) { HWY_DIRECT_SWITCH(hwy_rollout_direct_kernel, WPE) }
#undef HWY_DIRECT_SWITCH

hipError_t launch_step_direct(const DirectParams &dp, int num_envs, hipStream_t stream, int waves_per_eu, bool force_block_kernel,
                              int extra_lds) {
  if (wave_direct_applies(dp.s, force_block_kernel)) return launch_wave_direct(dp, num_envs, stream, waves_per_eu, extra_lds, false);
  switch (waves_per_eu) {
    case 1: return launch_step_direct_wpe<1>(dp, num_envs, stream);
    case 2: return launch_step_direct_wpe<2>(dp, num_envs, stream);
    case 3: return launch_step_direct_wpe<3>(dp, num_envs, stream);
    default: return launch_step_direct_wpe<4>(dp, num_envs, stream);
  }
}
hipError_t launch_rollout_direct(const DirectParams &dp, int num_envs, hipStream_t stream, int waves_per_eu, bool force_block_kernel,
                                 int extra_lds) {
  if (wave_direct_applies(dp.s, force_block_kernel)) return launch_wave_direct(dp, num_envs, stream, waves_per_eu, extra_lds, true);
  switch (waves_per_eu) {
    case 1: return launch_rollout_direct_wpe<1>(dp, num_envs, stream);
    case 2: return launch_rollout_direct_wpe<2>(dp, num_envs, stream);
    case 3: return launch_rollout_direct_wpe<3>(dp, num_envs, stream);
    default: return launch_rollout_direct_wpe<4>(dp, num_envs, stream);
  }
}
hipError_t launch_reset_direct(const DirectParams &dp, int num_envs, hipStream_t stream) {
  switch (waves_for(dp.s.N)) {
    case 1: return launch_dp(hwy_reset_direct_kernel<1>, 1, num_envs, stream, dp);
    case 2: return launch_dp(hwy_reset_direct_kernel<2>, 2, num_envs, stream, dp);
    case 3: return launch_dp(hwy_reset_direct_kernel<3>, 3, num_envs, stream, dp);
    case 4: return launch_dp(hwy_reset_direct_kernel<4>, 4, num_envs, stream, dp);
    default: return hipErrorInvalidValue;
  }
}

// workgroups of the direct-control step kernel the device holds at once (issue-priority turns pay only when the whole grid is resident)
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
  if (wave_direct_applies(p, force_block_kernel))
    return (p.flags & HWY_C_EGO_ONLY_COLLISIONS) ? resident(hwy_step_wave_direct_kernel<WPE, false>, 64, lds)
                                                 : resident(hwy_step_wave_direct_kernel<WPE, true>, 64, lds);
  switch (waves_for(p.N)) {
    case 1: return resident(hwy_step_direct_kernel<1, WPE>, 64);
    case 2: return resident(hwy_step_direct_kernel<2, WPE>, 128);
    case 3: return resident(hwy_step_direct_kernel<3, WPE>, 192);
    case 4: return resident(hwy_step_direct_kernel<4, WPE>, 256);
    default: return 0;
  }
}
int step_direct_resident_blocks(const StepParams &p, int waves_per_eu, bool force_block_kernel, int extra_lds) {
  switch (waves_per_eu) {
    case 1: return resident_wpe<1>(p, force_block_kernel, extra_lds);
    case 2: return resident_wpe<2>(p, force_block_kernel, extra_lds);
    case 3: return resident_wpe<3>(p, force_block_kernel, extra_lds);
    default: return resident_wpe<4>(p, force_block_kernel, extra_lds);
  }
}

}  // namespace hwy
