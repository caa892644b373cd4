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
#include "hwy_launch_family.h"

namespace hwy {

// the events of this thread's launches (hwy_launch_family.h: launch_kernel)
static thread_local hipEvent_t g_launch_start = nullptr, g_launch_stop = nullptr;
void set_launch_events(hipEvent_t start, hipEvent_t stop) { g_launch_start = start; g_launch_stop = stop; }
void get_launch_events(hipEvent_t *start, hipEvent_t *stop) { *start = g_launch_start; *stop = g_launch_stop; }

struct IdmFamily {
  using Params = StepParams;
  static const StepParams &step_params(const Params &a) { return a; }
  template <int WPE, bool FULL_SCAN> static auto step_wave() { return hwy_step_wave_kernel<WPE, FULL_SCAN>; }
  template <int WPE, bool FULL_SCAN> static auto rollout_wave() { return hwy_rollout_wave_kernel<WPE, FULL_SCAN>; }
  template <int NW, int WPE> static auto step_block() { return hwy_step_kernel<NW, WPE>; }
  template <int NW, int WPE> static auto rollout_block() { return hwy_rollout_kernel<NW, WPE>; }
  template <int NW> static auto reset_block() { return hwy_reset_kernel<NW>; }
};
using Idm = FamilyLaunch<IdmFamily>;

// 64 < N <= 256 with the Kinematics observation: ONE wavefront per environment, ceil(N / 64) vehicles per thread (hwy_wave2.h).
// Two per thread (BASELINE config 3's N = 101): 245 VGPRs, 15.7 KB of LDS, two resident wavefronts per SIMD.  Three / four per thread
// (N <= 192 / 256; round 5): 338 / 436 VGPRs without a spill, 23 / 30 KB of LDS, ONE wavefront per SIMD -- the same source, bit-identical
// to the workgroup kernel (tests/test_wide_kernel.py); the workgroup kernel (hwy_device.h) remains for the OccupancyGrid observation
// with N > 64 and behind hwy_config.tune_block_kernel.
static bool wide_kernel_applies(const StepParams &p, const Launch &l) {
  return p.N > 64 && p.N <= 256 && p.obs_type == HWY_OBS_KINEMATICS && !l.force_block_kernel;
}
// (one register-allocation variant per K: waves_per_eu does not count)
static hipError_t launch_wide(const StepParams &p, const Launch &l, bool rollout) {
  switch (waves_for(p.N)) {
    case 2: return rollout ? launch_kernel(hwy_rollout_wide_kernel<2, 2>, l.num_envs, 64, 0, l.stream, p)
                           : launch_kernel(hwy_step_wide_kernel<2, 2>, l.num_envs, 64, 0, l.stream, p);
    case 3: return rollout ? launch_kernel(hwy_rollout_wide_kernel<3, 1>, l.num_envs, 64, 0, l.stream, p)
                           : launch_kernel(hwy_step_wide_kernel<3, 1>, l.num_envs, 64, 0, l.stream, p);
    default: return rollout ? launch_kernel(hwy_rollout_wide_kernel<4, 1>, l.num_envs, 64, 0, l.stream, p)
                            : launch_kernel(hwy_step_wide_kernel<4, 1>, l.num_envs, 64, 0, l.stream, p);
  }
}
hipError_t launch_step(const StepParams &p, const Launch &l) {
  return wide_kernel_applies(p, l) ? launch_wide(p, l, false) : Idm::step(p, l, false);
}
hipError_t launch_rollout(const StepParams &p, const Launch &l) {
  return wide_kernel_applies(p, l) ? launch_wide(p, l, true) : Idm::step(p, l, true);
}
hipError_t launch_reset(const StepParams &p, const Launch &l) { return Idm::reset(p, l); }
hipError_t launch_observe(const StepParams &p, const Launch &l) {
  const int nw = waves_for(p.N);
  if (nw < 1 || nw > 4) return hipErrorInvalidValue;
  return dispatch_1_4(nw, [&](auto V) {
    constexpr int NW = decltype(V)::value;
    return launch_kernel(hwy_observe_kernel<NW>, l.num_envs, NW * 64, 0, l.stream, p);
  });
}
int step_resident_blocks(const StepParams &p, const Launch &l) {
  if (wide_kernel_applies(p, l)) return 0;  // (the wide kernel takes no issue-priority turns)
  return Idm::resident_blocks(p, l);
}

// road-network scenarios; <3, true>: the OccupancyGrid build (its own instantiation: hwy_net.h, net_observe<GRID>)
int step_resident_blocks(const NetParams &, const Launch &l) {
  return dispatch_1_4(l.waves_per_eu, [&](auto W) { return resident(hwy_net_step_kernel<decltype(W)::value>, 64); });
}
hipError_t launch_rollout(const NetParams &np, const Launch &l) {
  if (np.s.obs_type != HWY_OBS_KINEMATICS) return launch_kernel(hwy_net_rollout_kernel<3, true>, l.num_envs, 64, 0, l.stream, np);
  return dispatch_1_4(l.waves_per_eu, [&](auto W) {
    return launch_kernel(hwy_net_rollout_kernel<decltype(W)::value>, l.num_envs, 64, 0, l.stream, np);
  });
}
hipError_t launch_step(const NetParams &np, const Launch &l) {
  if (np.s.obs_type != HWY_OBS_KINEMATICS) return launch_kernel(hwy_net_step_kernel<3, true>, l.num_envs, 64, 0, l.stream, np);
  return dispatch_1_4(l.waves_per_eu, [&](auto W) {
    return launch_kernel(hwy_net_step_kernel<decltype(W)::value>, l.num_envs, 64, 0, l.stream, np);
  });
}
hipError_t launch_reset(const NetParams &np, const Launch &l) {
  if (np.s.obs_type != HWY_OBS_KINEMATICS) return launch_kernel(hwy_net_reset_kernel<1, true>, l.num_envs, 64, 0, l.stream, np);
  return launch_kernel(hwy_net_reset_kernel<1>, l.num_envs, 64, 0, l.stream, np);
}
hipError_t launch_observe(const NetParams &np, const Launch &l) {
  if (np.s.obs_type != HWY_OBS_KINEMATICS) return launch_kernel(hwy_net_observe_kernel<1, true>, l.num_envs, 64, 0, l.stream, np);
  return launch_kernel(hwy_net_observe_kernel<1>, l.num_envs, 64, 0, l.stream, np);
}

// intersection scenario: 32 threads for N <= 32 (64 with helper lanes), WPE 2 or 3 (158 VGPRs: 3 waves/SIMD is the most that fits)
template <int WPE>
static hipError_t launch_ix_step_wpe(const IxParams &ip, const Launch &l) {
  // with next-episode pre-warming the grid holds a second block per environment (hwy_ix.h: ix_prewarm)
  const int grid = (ip.shadow_meta && ip.s.autoreset && ip.s.full_step) ? 2 * l.num_envs : l.num_envs;
  if (ip.s.N <= 32 && ip.helpers) return launch_kernel(hwy_ix_step_kernel<WPE, 32, 64>, grid, 64, 0, l.stream, ip);
  if (ip.s.N <= 32) return launch_kernel(hwy_ix_step_kernel<WPE, 32>, grid, 32, 0, l.stream, ip);
  return launch_kernel(hwy_ix_step_kernel<2, 64>, grid, 64, 0, l.stream, ip);  // 24 KB of LDS: 2 waves/SIMD
}
template <int WPE>
static hipError_t launch_ix_rollout_wpe(const IxParams &ip, const Launch &l) {
  if (ip.s.N <= 32 && ip.helpers) return launch_kernel(hwy_ix_rollout_kernel<WPE, 32, 64>, l.num_envs, 64, 0, l.stream, ip);
  if (ip.s.N <= 32) return launch_kernel(hwy_ix_rollout_kernel<WPE, 32>, l.num_envs, 32, 0, l.stream, ip);
  return launch_kernel(hwy_ix_rollout_kernel<2, 64>, l.num_envs, 64, 0, l.stream, ip);
}
// ip.s.k_steps policy steps per launch (hwy_rollout_device); STEP blocks only
hipError_t launch_rollout(const IxParams &ip, const Launch &l) {
  return l.waves_per_eu >= 3 && l.waves_per_eu <= 4 ? launch_ix_rollout_wpe<3>(ip, l) : launch_ix_rollout_wpe<2>(ip, l);
}
hipError_t launch_step(const IxParams &ip, const Launch &l) {
  return l.waves_per_eu >= 3 && l.waves_per_eu <= 4 ? launch_ix_step_wpe<3>(ip, l) : launch_ix_step_wpe<2>(ip, l);
}
hipError_t launch_reset(const IxParams &ip, const Launch &l) {
  if (ip.s.N <= 32 && ip.helpers) return launch_kernel(hwy_ix_reset_kernel<2, 32, 64>, l.num_envs, 64, 0, l.stream, ip);
  if (ip.s.N <= 32) return launch_kernel(hwy_ix_reset_kernel<2, 32>, l.num_envs, 32, 0, l.stream, ip);
  return launch_kernel(hwy_ix_reset_kernel<2, 64>, l.num_envs, 64, 0, l.stream, ip);
}
hipError_t launch_observe(const IxParams &ip, const Launch &l) {
  if (ip.s.N <= 32) return launch_kernel(hwy_ix_observe_kernel<1, 32>, l.num_envs, 32, 0, l.stream, ip);
  return launch_kernel(hwy_ix_observe_kernel<1, 64>, l.num_envs, 64, 0, l.stream, ip);
}

__global__ void hwy_math_probe_kernel(int op, const double *in, double *out, long long n) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k < n) out[k] = math_probe(op, in[k]);
}
hipError_t launch_math_probe(int op, const double *in, double *out, long long n, hipStream_t stream) {
  return launch_kernel(hwy_math_probe_kernel, (unsigned)((n + 255) / 256), 256, 0, stream, op, in, out, n);
}

}  // namespace hwy
