// hwy_launch_family.h -- the host launch functions of ONE straight-road kernel family (IDM: hwy_kernels.hip, Linear traffic:
// hwy_kernels_linear.hip, direct ego control: hwy_kernels_direct.hip), written once.  A family is a trait:
//   using Params = ...;                                      the kernel argument (StepParams / LinearParams / DirectParams)
//   static const StepParams &step_params(const Params &);    the StepParams inside it
//   step_wave<WPE, FULL_SCAN>() / rollout_wave<WPE, FULL_SCAN>()   the one-wavefront kernels (hwy_wave.h, N <= 64)
//   step_block<NW, WPE>() / rollout_block<NW, WPE>() / reset_block<NW>()   the workgroup kernels (hwy_device.h, NW wavefronts)
// each returning the address of the kernel.  Host code only: it is included by the kernel translation units after the kernel headers.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <type_traits>

#include "hwy_launch.h"

namespace hwy {

void get_launch_events(hipEvent_t *start, hipEvent_t *stop);  // hwy_kernels.hip: the events of this thread's launches (hwy_profile_*)

static inline int waves_for(int n_vehicles) { return (n_vehicles + 63) / 64; }

// fn(std::integral_constant<int, v>{}) for a run-time v in 1 .. 4 (anything else: 4, the register-allocation variants' default):
// every choice of a kernel instantiation by waves_per_eu or by wavefronts per environment goes through here
template <typename Fn>
static auto dispatch_1_4(int v, Fn &&fn) {
  switch (v) {
    case 1: return fn(std::integral_constant<int, 1>{});
    case 2: return fn(std::integral_constant<int, 2>{});
    case 3: return fn(std::integral_constant<int, 3>{});
    default: return fn(std::integral_constant<int, 4>{});
  }
}

// Kernel timing (hwy_profile_enable): every launch goes through hipExtLaunchKernelGGL, which records the DISPATCH's own begin and
// end timestamps into the two events it is given -- the same clock readings rocprofv3 --kernel-trace reports, with no stream
// overhead between them (events recorded around a launch with hipEventRecord also measure ~3 us of command processing).
// Null events (the normal case): a plain launch.
template <typename K, typename... A>
static hipError_t launch_kernel(K kernel, unsigned grid, int block, int lds, hipStream_t stream, const A &...a) {
  hipEvent_t start, stop;
  get_launch_events(&start, &stop);
  hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, stream, start, stop, 0, a...);
  return hipGetLastError();
}

// How many workgroups of a kernel the device holds at once (occupancy x compute units): the issue-priority turns (hwy_wave.h:
// WaveTurn) only pay when the whole grid is resident.
template <typename K>
static int resident(K kernel, int block, int lds = 0) {
  int per_cu = 0, dev = 0;
  hipDeviceProp_t prop;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, lds) != hipSuccess) return 0;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
  return per_cu * prop.multiProcessorCount;
}

template <typename F>
struct FamilyLaunch {
  using P = typename F::Params;
  // N <= 64: one wavefront per environment (hwy_wave.h); otherwise ceil(N / 64) wavefronts per workgroup (hwy_device.h)
  static bool wave_applies(const StepParams &p, const Launch &l) { return p.N <= 64 && !l.force_block_kernel; }
  // one policy step, or (rollout) p.k_steps of them in one launch; the one-wavefront ROLLOUT kernel has a waves_per_eu of its own
  static hipError_t step(const P &a, const Launch &l, bool rollout) {
    const StepParams &p = F::step_params(a);
    const int nw = waves_for(p.N);
    if (wave_applies(p, l)) {
      // FULL_SCAN = every vehicle checks collisions (highway-v0).  lds = hwy_config.tune_extra_lds: dynamic LDS reserved per
      // workgroup, i.e. fewer resident wavefronts per SIMD, so that part of the grid is dispatched as wavefronts retire (the
      // hardware then balances unevenly loaded SIMDs)
      const bool fast = (p.flags & HWY_C_EGO_ONLY_COLLISIONS) != 0;
      return dispatch_1_4(rollout ? l.rollout_waves_per_eu : l.waves_per_eu, [&](auto W) {
        constexpr int WPE = decltype(W)::value;
        if (rollout) return fast ? launch_kernel(F::template rollout_wave<WPE, false>(), l.num_envs, 64, l.extra_lds, l.stream, a)
                                 : launch_kernel(F::template rollout_wave<WPE, true>(), l.num_envs, 64, l.extra_lds, l.stream, a);
        return fast ? launch_kernel(F::template step_wave<WPE, false>(), l.num_envs, 64, l.extra_lds, l.stream, a)
                    : launch_kernel(F::template step_wave<WPE, true>(), l.num_envs, 64, l.extra_lds, l.stream, a);
      });
    }
    if (nw < 1 || nw > 4) return hipErrorInvalidValue;
    return dispatch_1_4(l.waves_per_eu, [&](auto W) {  // WPE = the register-allocation variant (hwy_engine.hip: waves_per_eu)
      return dispatch_1_4(nw, [&](auto V) {
        constexpr int WPE = decltype(W)::value, NW = decltype(V)::value;
        return rollout ? launch_kernel(F::template rollout_block<NW, WPE>(), l.num_envs, NW * 64, 0, l.stream, a)
                       : launch_kernel(F::template step_block<NW, WPE>(), l.num_envs, NW * 64, 0, l.stream, a);
      });
    });
  }
  static hipError_t reset(const P &a, const Launch &l) {
    const int nw = waves_for(F::step_params(a).N);
    if (nw < 1 || nw > 4) return hipErrorInvalidValue;
    return dispatch_1_4(nw, [&](auto V) {
      constexpr int NW = decltype(V)::value;
      return launch_kernel(F::template reset_block<NW>(), l.num_envs, NW * 64, 0, l.stream, a);
    });
  }
  // workgroups of the step kernel this launch would run that the device holds at once (0 = unknown)
  static int resident_blocks(const P &a, const Launch &l) {
    const StepParams &p = F::step_params(a);
    const int nw = waves_for(p.N);
    if (!wave_applies(p, l) && (nw < 1 || nw > 4)) return 0;
    return dispatch_1_4(l.waves_per_eu, [&](auto W) {
      constexpr int WPE = decltype(W)::value;
      if (wave_applies(p, l))
        return (p.flags & HWY_C_EGO_ONLY_COLLISIONS) ? resident(F::template step_wave<WPE, false>(), 64, l.extra_lds)
                                                     : resident(F::template step_wave<WPE, true>(), 64, l.extra_lds);
      // workgroup kernel: turns by workgroup (hwy_device.h: wave_turn_init_workgroup)
      return dispatch_1_4(nw, [&](auto V) { return resident(F::template step_block<decltype(V)::value, WPE>(), decltype(V)::value * 64); });
    });
  }
};

}  // namespace hwy
