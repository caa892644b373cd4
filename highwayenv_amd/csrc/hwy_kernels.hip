// hwy_kernels.hip -- gfx950 translation unit: instantiates the fused step / reset /
// observe kernels of hwy_device.h and exposes plain launch functions to the C-ABI host
// (hwy_engine.hip).  Build: highwayenv_amd/build.py (hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=on ...).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#define HWY_HAVE_SETPRIO 1  // s_setprio / s_memtime / s_getreg exist on the device (not in the CPU emulation of tests/emu)
#include "hwy_device.h"
#include "hwy_wave.h"
#include "hwy_wave2.h"
#include "hwy_net.h"
#include "hwy_ix.h"
#include "hwy_launch.h"

namespace hwy {

// Kernel timing (hwy_profile_enable): every launch goes through hipExtLaunchKernelGGL, which records the DISPATCH's own begin and
// end timestamps into the two events it is given -- the same clock readings rocprofv3 --kernel-trace reports, with no stream
// overhead between them (events recorded around a launch with hipEventRecord also measure ~3 us of command processing).
// Null events (the normal case): a plain launch.
static thread_local hipEvent_t g_launch_start = nullptr, g_launch_stop = nullptr;
void set_launch_events(hipEvent_t start, hipEvent_t stop) { g_launch_start = start; g_launch_stop = stop; }
void get_launch_events(hipEvent_t *start, hipEvent_t *stop) { *start = g_launch_start; *stop = g_launch_stop; }
#define HWY_LAUNCH(KERNEL, grid, block, lds, stream, ...) \
  hipExtLaunchKernelGGL(KERNEL, grid, block, lds, stream, ::hwy::g_launch_start, ::hwy::g_launch_stop, 0, __VA_ARGS__)

static inline int waves_for(int n_vehicles) { return (n_vehicles + 63) / 64; }

#define HWY_DISPATCH(KERNEL)                                                                  \
  switch (waves_for(p.N)) {                                                                   \
    case 1: HWY_LAUNCH(KERNEL<1>, dim3(num_envs), dim3(64), 0, stream, p); break;     \
    case 2: HWY_LAUNCH(KERNEL<2>, dim3(num_envs), dim3(128), 0, stream, p); break;    \
    case 3: HWY_LAUNCH(KERNEL<3>, dim3(num_envs), dim3(192), 0, stream, p); break;    \
    case 4: HWY_LAUNCH(KERNEL<4>, dim3(num_envs), dim3(256), 0, stream, p); break;    \
    default: return hipErrorInvalidValue;                                                     \
  }                                                                                           \
  return hipGetLastError();

template <int WPE>
static hipError_t launch_step_wpe(const StepParams &p, int num_envs, hipStream_t stream) {
  switch (waves_for(p.N)) {
    case 1: HWY_LAUNCH((hwy_step_kernel<1, WPE>), dim3(num_envs), dim3(64), 0, stream, p); break;
    case 2: HWY_LAUNCH((hwy_step_kernel<2, WPE>), dim3(num_envs), dim3(128), 0, stream, p); break;
    case 3: HWY_LAUNCH((hwy_step_kernel<3, WPE>), dim3(num_envs), dim3(192), 0, stream, p); break;
    case 4: HWY_LAUNCH((hwy_step_kernel<4, WPE>), dim3(num_envs), dim3(256), 0, stream, p); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
template <int WPE>
static hipError_t launch_block_rollout_wpe(const StepParams &p, int num_envs, hipStream_t stream) {
  switch (waves_for(p.N)) {
    case 1: HWY_LAUNCH((hwy_rollout_kernel<1, WPE>), dim3(num_envs), dim3(64), 0, stream, p); break;
    case 2: HWY_LAUNCH((hwy_rollout_kernel<2, WPE>), dim3(num_envs), dim3(128), 0, stream, p); break;
    case 3: HWY_LAUNCH((hwy_rollout_kernel<3, WPE>), dim3(num_envs), dim3(192), 0, stream, p); break;
    case 4: HWY_LAUNCH((hwy_rollout_kernel<4, WPE>), dim3(num_envs), dim3(256), 0, stream, p); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
template <int WPE>
static hipError_t launch_wave_wpe(const StepParams &p, int num_envs, hipStream_t stream, int lds) {
  // lds = hwy_config.tune_extra_lds: dynamic LDS reserved per workgroup, i.e. fewer resident wavefronts per SIMD, so that part
  // of the grid is dispatched as wavefronts retire (the hardware then balances unevenly loaded SIMDs)
  if (p.flags & HWY_C_EGO_ONLY_COLLISIONS)
    HWY_LAUNCH((hwy_step_wave_kernel<WPE, false>), dim3(num_envs), dim3(64), lds, stream, p);
  else
    HWY_LAUNCH((hwy_step_wave_kernel<WPE, true>), dim3(num_envs), dim3(64), lds, stream, p);
  return hipGetLastError();
}
template <int WPE>
static hipError_t launch_rollout_wpe(const StepParams &p, int num_envs, hipStream_t stream, int lds) {
  if (p.flags & HWY_C_EGO_ONLY_COLLISIONS)
    HWY_LAUNCH((hwy_rollout_wave_kernel<WPE, false>), dim3(num_envs), dim3(64), lds, stream, p);
  else
    HWY_LAUNCH((hwy_rollout_wave_kernel<WPE, true>), dim3(num_envs), dim3(64), lds, stream, p);
  return hipGetLastError();
}
// 64 < N <= 256 with the Kinematics observation: ONE wavefront per environment, ceil(N / 64) vehicles per thread (hwy_wave2.h).
// Two per thread (BASELINE config 3's N = 101): 245 VGPRs, 15.7 KB of LDS, two resident wavefronts per SIMD.  Three / four per thread
// (N <= 192 / 256; round 5): 338 / 436 VGPRs without a spill, 23 / 30 KB of LDS, ONE wavefront per SIMD -- the same source, bit-identical
// to the workgroup kernel (tests/test_wide_kernel.py); the workgroup kernel (hwy_device.h) remains for the OccupancyGrid observation
// with N > 64 and behind hwy_config.tune_block_kernel.
bool wide_kernel_applies(const StepParams &p, bool force_block_kernel) {
  return p.N > 64 && p.N <= 256 && p.obs_type == HWY_OBS_KINEMATICS && !force_block_kernel;
}
static hipError_t launch_wide(const StepParams &p, int num_envs, hipStream_t stream, int waves_per_eu) {
  (void)waves_per_eu;  // (one register-allocation variant per K)
  switch (waves_for(p.N)) {
    case 2: HWY_LAUNCH((hwy_step_wide_kernel<2, 2>), dim3(num_envs), dim3(64), 0, stream, p); break;
    case 3: HWY_LAUNCH((hwy_step_wide_kernel<3, 1>), dim3(num_envs), dim3(64), 0, stream, p); break;
    default: HWY_LAUNCH((hwy_step_wide_kernel<4, 1>), dim3(num_envs), dim3(64), 0, stream, p); break;
  }
  return hipGetLastError();
}
static hipError_t launch_wide_rollout(const StepParams &p, int num_envs, hipStream_t stream, int waves_per_eu) {
  (void)waves_per_eu;
  switch (waves_for(p.N)) {
    case 2: HWY_LAUNCH((hwy_rollout_wide_kernel<2, 2>), dim3(num_envs), dim3(64), 0, stream, p); break;
    case 3: HWY_LAUNCH((hwy_rollout_wide_kernel<3, 1>), dim3(num_envs), dim3(64), 0, stream, p); break;
    default: HWY_LAUNCH((hwy_rollout_wide_kernel<4, 1>), dim3(num_envs), dim3(64), 0, stream, p); break;
  }
  return hipGetLastError();
}
// hwy_rollout_device on the straight-road kernels: p.k_steps policy steps in one launch -- the one-wavefront kernel for N <= 64,
// the workgroup kernel otherwise (or when forced).
hipError_t launch_rollout(const StepParams &p, int num_envs, hipStream_t stream, int waves_per_eu, int extra_lds,
                          bool force_block_kernel, int block_waves_per_eu) {
  if (wide_kernel_applies(p, force_block_kernel)) return launch_wide_rollout(p, num_envs, stream, block_waves_per_eu);
  if (p.N > 64 || force_block_kernel) {
    switch (block_waves_per_eu) {
      case 1: return launch_block_rollout_wpe<1>(p, num_envs, stream);
      case 2: return launch_block_rollout_wpe<2>(p, num_envs, stream);
      case 3: return launch_block_rollout_wpe<3>(p, num_envs, stream);
      default: return launch_block_rollout_wpe<4>(p, num_envs, stream);
    }
  }
  switch (waves_per_eu) {
    case 1: return launch_rollout_wpe<1>(p, num_envs, stream, extra_lds);
    case 2: return launch_rollout_wpe<2>(p, num_envs, stream, extra_lds);
    case 3: return launch_rollout_wpe<3>(p, num_envs, stream, extra_lds);
    default: return launch_rollout_wpe<4>(p, num_envs, stream, extra_lds);
  }
}
// N <= 64: one wavefront per environment (hwy_wave.h); otherwise ceil(N/64) wavefronts per workgroup.
hipError_t launch_step(const StepParams &p, int num_envs, hipStream_t stream, int waves_per_eu, bool force_block_kernel,
                       int extra_lds) {
  if (wide_kernel_applies(p, force_block_kernel)) return launch_wide(p, num_envs, stream, waves_per_eu);
  if (p.N <= 64 && !force_block_kernel) {
    switch (waves_per_eu) {
      case 1: return launch_wave_wpe<1>(p, num_envs, stream, extra_lds);
      case 2: return launch_wave_wpe<2>(p, num_envs, stream, extra_lds);
      case 3: return launch_wave_wpe<3>(p, num_envs, stream, extra_lds);
      default: return launch_wave_wpe<4>(p, num_envs, stream, extra_lds);
    }
  }
  switch (waves_per_eu) {
    case 1: return launch_step_wpe<1>(p, num_envs, stream);
    case 2: return launch_step_wpe<2>(p, num_envs, stream);
    case 3: return launch_step_wpe<3>(p, num_envs, stream);
    default: return launch_step_wpe<4>(p, num_envs, stream);
  }
}
// How many workgroups of the step kernel a launch of this engine can hold at once (occupancy x compute units): the
// issue-priority turns (hwy_wave.h: WaveTurn) only pay when the whole grid is resident.
template <typename K>
static int resident_blocks(K kernel, int block, int dyn_lds) {
  int per_cu = 0, dev = 0;
  hipDeviceProp_t prop;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, dyn_lds) != hipSuccess) return 0;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
  return per_cu * prop.multiProcessorCount;
}
template <int WPE>
static int block_resident_wpe(int n) {
  switch (waves_for(n)) {
    case 1: return resident_blocks(hwy_step_kernel<1, WPE>, 64, 0);
    case 2: return resident_blocks(hwy_step_kernel<2, WPE>, 128, 0);
    case 3: return resident_blocks(hwy_step_kernel<3, WPE>, 192, 0);
    case 4: return resident_blocks(hwy_step_kernel<4, WPE>, 256, 0);
    default: return 0;
  }
}
int step_resident_blocks(const StepParams &p, int waves_per_eu, bool force_block_kernel, int extra_lds) {
  if (wide_kernel_applies(p, force_block_kernel)) return 0;  // (the wide kernel takes no issue-priority turns)
  if (p.N > 64 || force_block_kernel) {  // workgroup kernel: turns by workgroup (hwy_device.h: wave_turn_init_workgroup)
    switch (waves_per_eu) {
      case 1: return block_resident_wpe<1>(p.N);
      case 2: return block_resident_wpe<2>(p.N);
      case 3: return block_resident_wpe<3>(p.N);
      default: return block_resident_wpe<4>(p.N);
    }
  }
  const bool fast = (p.flags & HWY_C_EGO_ONLY_COLLISIONS) != 0;
  switch (waves_per_eu) {
    case 1: return fast ? resident_blocks(hwy_step_wave_kernel<1, false>, 64, extra_lds) : resident_blocks(hwy_step_wave_kernel<1, true>, 64, extra_lds);
    case 2: return fast ? resident_blocks(hwy_step_wave_kernel<2, false>, 64, extra_lds) : resident_blocks(hwy_step_wave_kernel<2, true>, 64, extra_lds);
    case 3: return fast ? resident_blocks(hwy_step_wave_kernel<3, false>, 64, extra_lds) : resident_blocks(hwy_step_wave_kernel<3, true>, 64, extra_lds);
    default: return fast ? resident_blocks(hwy_step_wave_kernel<4, false>, 64, extra_lds) : resident_blocks(hwy_step_wave_kernel<4, true>, 64, extra_lds);
  }
}
int net_step_resident_blocks(int waves_per_eu) {
  switch (waves_per_eu) {
    case 1: return resident_blocks(hwy_net_step_kernel<1>, 64, 0);
    case 2: return resident_blocks(hwy_net_step_kernel<2>, 64, 0);
    case 3: return resident_blocks(hwy_net_step_kernel<3>, 64, 0);
    default: return resident_blocks(hwy_net_step_kernel<4>, 64, 0);
  }
}
hipError_t launch_net_rollout(const NetParams &np, int num_envs, hipStream_t stream, int waves_per_eu) {
  if (np.s.obs_type != HWY_OBS_KINEMATICS) {
    HWY_LAUNCH((hwy_net_rollout_kernel<3, true>), dim3(num_envs), dim3(64), 0, stream, np);
    return hipGetLastError();
  }
  switch (waves_per_eu) {
    case 1: HWY_LAUNCH((hwy_net_rollout_kernel<1>), dim3(num_envs), dim3(64), 0, stream, np); break;
    case 2: HWY_LAUNCH((hwy_net_rollout_kernel<2>), dim3(num_envs), dim3(64), 0, stream, np); break;
    case 3: HWY_LAUNCH((hwy_net_rollout_kernel<3>), dim3(num_envs), dim3(64), 0, stream, np); break;
    default: HWY_LAUNCH((hwy_net_rollout_kernel<4>), dim3(num_envs), dim3(64), 0, stream, np); break;
  }
  return hipGetLastError();
}
hipError_t launch_net_step(const NetParams &np, int num_envs, hipStream_t stream, int waves_per_eu) {
  if (np.s.obs_type != HWY_OBS_KINEMATICS) {  // the OccupancyGrid build (its own instantiation: hwy_net.h, net_observe<GRID>)
    HWY_LAUNCH((hwy_net_step_kernel<3, true>), dim3(num_envs), dim3(64), 0, stream, np);
    return hipGetLastError();
  }
  switch (waves_per_eu) {
    case 1: HWY_LAUNCH((hwy_net_step_kernel<1>), dim3(num_envs), dim3(64), 0, stream, np); break;
    case 2: HWY_LAUNCH((hwy_net_step_kernel<2>), dim3(num_envs), dim3(64), 0, stream, np); break;
    case 3: HWY_LAUNCH((hwy_net_step_kernel<3>), dim3(num_envs), dim3(64), 0, stream, np); break;
    default: HWY_LAUNCH((hwy_net_step_kernel<4>), dim3(num_envs), dim3(64), 0, stream, np); break;
  }
  return hipGetLastError();
}
hipError_t launch_net_reset(const NetParams &np, int num_envs, hipStream_t stream) {
  if (np.s.obs_type != HWY_OBS_KINEMATICS) HWY_LAUNCH((hwy_net_reset_kernel<1, true>), dim3(num_envs), dim3(64), 0, stream, np);
  else HWY_LAUNCH((hwy_net_reset_kernel<1>), dim3(num_envs), dim3(64), 0, stream, np);
  return hipGetLastError();
}
hipError_t launch_net_observe(const NetParams &np, int num_envs, hipStream_t stream) {
  if (np.s.obs_type != HWY_OBS_KINEMATICS) HWY_LAUNCH((hwy_net_observe_kernel<1, true>), dim3(num_envs), dim3(64), 0, stream, np);
  else HWY_LAUNCH((hwy_net_observe_kernel<1>), dim3(num_envs), dim3(64), 0, stream, np);
  return hipGetLastError();
}
template <int WPE>
static void launch_ix_step_wpe(const IxParams &ip, int num_envs, hipStream_t stream) {
  // with next-episode pre-warming the grid holds a second block per environment (hwy_ix.h: ix_prewarm)
  const int grid = (ip.shadow_meta && ip.s.autoreset && ip.s.full_step) ? 2 * num_envs : num_envs;
  if (ip.s.N <= 32 && ip.helpers) HWY_LAUNCH((hwy_ix_step_kernel<WPE, 32, 64>), dim3(grid), dim3(64), 0, stream, ip);
  else if (ip.s.N <= 32) HWY_LAUNCH((hwy_ix_step_kernel<WPE, 32>), dim3(grid), dim3(32), 0, stream, ip);
  else HWY_LAUNCH((hwy_ix_step_kernel<2, 64>), dim3(grid), dim3(64), 0, stream, ip);  // 24 KB of LDS: 2 waves/SIMD
}
template <int WPE>
static void launch_ix_rollout_wpe(const IxParams &ip, int num_envs, hipStream_t stream) {
  if (ip.s.N <= 32 && ip.helpers) HWY_LAUNCH((hwy_ix_rollout_kernel<WPE, 32, 64>), dim3(num_envs), dim3(64), 0, stream, ip);
  else if (ip.s.N <= 32) HWY_LAUNCH((hwy_ix_rollout_kernel<WPE, 32>), dim3(num_envs), dim3(32), 0, stream, ip);
  else HWY_LAUNCH((hwy_ix_rollout_kernel<2, 64>), dim3(num_envs), dim3(64), 0, stream, ip);
}
// ip.s.k_steps policy steps per launch (hwy_rollout_device); STEP blocks only
hipError_t launch_ix_rollout(const IxParams &ip, int num_envs, hipStream_t stream, int waves_per_eu) {
  switch (waves_per_eu) {
    case 3: case 4: launch_ix_rollout_wpe<3>(ip, num_envs, stream); break;
    default: launch_ix_rollout_wpe<2>(ip, num_envs, stream); break;
  }
  return hipGetLastError();
}
hipError_t launch_ix_step(const IxParams &ip, int num_envs, hipStream_t stream, int waves_per_eu) {
  switch (waves_per_eu) {
    case 3: case 4: launch_ix_step_wpe<3>(ip, num_envs, stream); break;  // (158 VGPRs: 3 waves/SIMD is the most that fits)
    default: launch_ix_step_wpe<2>(ip, num_envs, stream); break;
  }
  return hipGetLastError();
}
hipError_t launch_ix_reset(const IxParams &ip, int num_envs, hipStream_t stream) {
  if (ip.s.N <= 32 && ip.helpers) HWY_LAUNCH((hwy_ix_reset_kernel<2, 32, 64>), dim3(num_envs), dim3(64), 0, stream, ip);
  else if (ip.s.N <= 32) HWY_LAUNCH((hwy_ix_reset_kernel<2, 32>), dim3(num_envs), dim3(32), 0, stream, ip);
  else HWY_LAUNCH((hwy_ix_reset_kernel<2, 64>), dim3(num_envs), dim3(64), 0, stream, ip);
  return hipGetLastError();
}
hipError_t launch_ix_observe(const IxParams &ip, int num_envs, hipStream_t stream) {
  if (ip.s.N <= 32) HWY_LAUNCH((hwy_ix_observe_kernel<1, 32>), dim3(num_envs), dim3(32), 0, stream, ip);
  else HWY_LAUNCH((hwy_ix_observe_kernel<1, 64>), dim3(num_envs), dim3(64), 0, stream, ip);
  return hipGetLastError();
}
__global__ void hwy_math_probe_kernel(int op, const double *in, double *out, long long n) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k < n) out[k] = math_probe(op, in[k]);
}
hipError_t launch_math_probe(int op, const double *in, double *out, long long n, hipStream_t stream) {
  HWY_LAUNCH(hwy_math_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, op, in, out, n);
  return hipGetLastError();
}
hipError_t launch_reset(const StepParams &p, int num_envs, hipStream_t stream) { HWY_DISPATCH(hwy_reset_kernel) }
hipError_t launch_observe(const StepParams &p, int num_envs, hipStream_t stream) { HWY_DISPATCH(hwy_observe_kernel) }

}  // namespace hwy
