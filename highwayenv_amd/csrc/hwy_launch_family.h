// hwy_launch_family.h -- (kernel arguments, Launch) -> (kernel instantiation, grid, block, LDS) of the straight-road kernel
// families, written ONCE for the product and for the CPU emulation of tests/emu.  hwy_launch_rules.h has the rest of the rules (the
// wide kernel, the road-network and the intersection scenarios).  Host code only, generic over the thing that launches -- a backend B
// with three members:
//   B::launch(kernel, grid, block, lds, const Launch &, args...)   enqueue / run the kernel
//   B::resident(kernel, block, lds)                                workgroups of it the device holds at once (0 = unknown)
//   B::pick_wpe(v, fn)                                             fn(std::integral_constant<int, W>{}) for the waves-per-EU variant
//                                                                  W of a run-time v: the register-allocation builds of one kernel
// hwy_launch.h: HipBackend (hipExtLaunchKernelGGL, the occupancy query, W = v); tests/emu/emu_straight.h: EmuBackend (emu::launch, 0,
// W = 1 -- the variants are the same source, the emulation compiles one).
// A family is a trait:
//   using Params = ...;                                      the kernel argument (StepParams / LinearParams / DirectParams)
//   step_params(Params &)                                    the StepParams inside it
//   step_wave<WPE, FULL_SCAN>() / rollout_wave<WPE, FULL_SCAN>()   the one-wavefront kernels (hwy_wave.h, N <= 64)
//   step_block<NW, WPE>() / rollout_block<NW, WPE>() / reset_block<NW>() / respawn_block<NW>()   the workgroup kernels (hwy_device.h,
//                                                                  NW wavefronts); respawn_wave(): hwy_wave.h's
// each returning the address of the kernel (taking it is what instantiates the kernel: a translation unit holds the kernels of the
// families it launches and no others).
// hipError_t / hipStream_t / hipEvent_t come from the HIP runtime (the emulation: from hip_emu.h).
#pragma once
#include <type_traits>

#include "hwy_device.h"
#include "hwy_wave.h"
#include "hwy_params.h"

namespace hwy {

// What the engine decides about a launch, whatever the family.  waves_per_eu: the register-allocation variant of the step kernel;
// rollout_waves_per_eu: that of the ONE-WAVEFRONT rollout kernel of the straight-road families (their workgroup rollout kernel
// takes waves_per_eu, the wide kernel has one variant per size); force_block_kernel / extra_lds: hwy_config.tune_block_kernel /
// tune_extra_lds as resolved by hwy_create (straight-road families only); start / stop: the events the launch records its
// dispatch's begin / end timestamps into (hwy_profile_*, the turn tuner), null = a plain launch
struct Launch {
  int num_envs;
  hipStream_t stream;
  int waves_per_eu, rollout_waves_per_eu;
  bool force_block_kernel;
  int extra_lds;
  hipEvent_t start, stop;
};

static inline int waves_for(int n_vehicles) { return (n_vehicles + 63) / 64; }

// ---- shapes of the one-wavefront step kernel (hwy_wave.h: FixedShape) -------------------------------------------------------
// Whether launches may take a shape kernel, and which one the last step launch of a straight-road family took (0 = the generic
// kernel): ONE state per library, behind the two exports below -- the product's library and the CPU emulation's carry the same
// two symbols, because this header is what both are built from.  Initially on, unless the environment says HWY_STEP_SHAPES=0
// (read once, at the first use).
struct StepShapeState {
  bool enabled;
  int last;
};
inline StepShapeState &step_shape_state() {
  static StepShapeState s = [] {
    const char *v = std::getenv("HWY_STEP_SHAPES");
    return StepShapeState{!(v && v[0] == '0' && v[1] == 0), 0};
  }();
  return s;
}
// The shape whose EVERY fixed field equals the StepParams of THIS launch (full_step, autoreset and the pointers change from call to
// call), or 0: the generic kernel -- a frames-only call, a call without actions, an engine before hwy_set_autoreset, a multi-step
// launch, any other configuration.  IDM traffic with meta-actions on the one-wavefront kernel only.
inline int step_shape_of(const StepParams &p, const Launch &l, bool rollout) {
  if (!step_shape_state().enabled || rollout || p.N > 64 || l.force_block_kernel) return 0;
  if (FastShape3::matches(p)) return FastShape3::ID;
  if (FastShape4::matches(p)) return FastShape4::ID;
  if (V0Shape4::matches(p)) return V0Shape4::ID;
  return 0;
}
// the launch of shape `id` (> 0, from step_shape_of) in the register-allocation build the Launch asks for.  With the HIP backend it
// is instantiated in hwy_kernels_shapes.hip alone (hwy_launch.h declares it extern): the shape kernels are a translation unit of
// their own.
template <typename B> hipError_t launch_step_shape(int id, const StepParams &p, const Launch &l) {
  step_shape_state().last = id;
  return B::pick_wpe(l.waves_per_eu, [&](auto W) {
    constexpr int WPE = decltype(W)::value;
    switch (id) {
      case FastShape3::ID: return B::launch(hwy_shape_wave_kernel<FastShape3, WPE>, l.num_envs, 64, l.extra_lds, l, p);
      case FastShape4::ID: return B::launch(hwy_shape_wave_kernel<FastShape4, WPE>, l.num_envs, 64, l.extra_lds, l, p);
      case V0Shape4::ID: return B::launch(hwy_shape_wave_kernel<V0Shape4, WPE>, l.num_envs, 64, l.extra_lds, l, p);
      default: return hipErrorInvalidValue;
    }
  });
}

// fn(std::integral_constant<int, v>{}) for a run-time v in 1 .. 4 (anything else: 4, the register-allocation variants' default)
template <typename Fn>
static auto dispatch_1_4(int v, Fn &&fn) {
  switch (v) {
    case 1: return fn(std::integral_constant<int, 1>{});
    case 2: return fn(std::integral_constant<int, 2>{});
    case 3: return fn(std::integral_constant<int, 3>{});
    default: return fn(std::integral_constant<int, 4>{});
  }
}

struct IdmFamily {  // IDM traffic, meta-actions (hwy_kernels.hip)
  using Params = StepParams;
  static StepParams &step_params(Params &a) { return a; }
  static const StepParams &step_params(const Params &a) { return a; }
  template <int WPE, bool FULL_SCAN> static auto step_wave() { return hwy_step_wave_kernel<WPE, FULL_SCAN>; }
  template <int WPE, bool FULL_SCAN> static auto rollout_wave() { return hwy_rollout_wave_kernel<WPE, FULL_SCAN>; }
  template <int NW, int WPE> static auto step_block() { return hwy_step_kernel<NW, WPE>; }
  template <int NW, int WPE> static auto rollout_block() { return hwy_rollout_kernel<NW, WPE>; }
  template <int NW> static auto reset_block() { return hwy_reset_kernel<NW>; }
  template <int NW> static auto respawn_block() { return hwy_respawn_kernel<NW>; }
  static auto respawn_wave() { return hwy_respawn_wave_kernel<1>; }
};
struct LinearFamily {  // hwy_config.traffic_model == HWY_TRAFFIC_LINEAR (hwy_kernels_linear.hip)
  using Params = LinearParams;
  static StepParams &step_params(Params &a) { return a.s; }
  static const StepParams &step_params(const Params &a) { return a.s; }
  template <int WPE, bool FULL_SCAN> static auto step_wave() { return hwy_step_wave_linear_kernel<WPE, FULL_SCAN>; }
  template <int WPE, bool FULL_SCAN> static auto rollout_wave() { return hwy_rollout_wave_linear_kernel<WPE, FULL_SCAN>; }
  template <int NW, int WPE> static auto step_block() { return hwy_step_linear_kernel<NW, WPE>; }
  template <int NW, int WPE> static auto rollout_block() { return hwy_rollout_linear_kernel<NW, WPE>; }
  template <int NW> static auto reset_block() { return hwy_reset_linear_kernel<NW>; }
  template <int NW> static auto respawn_block() { return hwy_respawn_linear_kernel<NW>; }
  static auto respawn_wave() { return hwy_respawn_wave_linear_kernel<1>; }
};
struct DirectFamily {  // hwy_config.ego_control == HWY_EGO_DIRECT (hwy_kernels_direct.hip)
  using Params = DirectParams;
  static StepParams &step_params(Params &a) { return a.s; }
  static const StepParams &step_params(const Params &a) { return a.s; }
  template <int WPE, bool FULL_SCAN> static auto step_wave() { return hwy_step_wave_direct_kernel<WPE, FULL_SCAN>; }
  template <int WPE, bool FULL_SCAN> static auto rollout_wave() { return hwy_rollout_wave_direct_kernel<WPE, FULL_SCAN>; }
  template <int NW, int WPE> static auto step_block() { return hwy_step_direct_kernel<NW, WPE>; }
  template <int NW, int WPE> static auto rollout_block() { return hwy_rollout_direct_kernel<NW, WPE>; }
  template <int NW> static auto reset_block() { return hwy_reset_direct_kernel<NW>; }
  template <int NW> static auto respawn_block() { return hwy_respawn_direct_kernel<NW>; }
  static auto respawn_wave() { return hwy_respawn_wave_direct_kernel<1>; }
};

template <typename F, typename B>
struct FamilyLaunch {
  using P = typename F::Params;
  // N <= 64: one wavefront per environment (hwy_wave.h); otherwise ceil(N / 64) wavefronts per workgroup (hwy_device.h)
  static bool wave_applies(const StepParams &p, const Launch &l) { return p.N <= 64 && !l.force_block_kernel; }
  // one policy step, or (rollout) p.k_steps of them in one launch; the one-wavefront ROLLOUT kernel has a waves_per_eu of its own
  static hipError_t step(const P &a, const Launch &l, bool rollout) {
    const StepParams &p = F::step_params(a);
    const int nw = waves_for(p.N);
    step_shape_state().last = 0;  // (a shape launch does not come through here: hwy_launch_rules.h, select_step)
    if (wave_applies(p, l)) {
      // FULL_SCAN = every vehicle checks collisions (highway-v0).  lds = hwy_config.tune_extra_lds: dynamic LDS reserved per
      // workgroup, i.e. fewer resident wavefronts per SIMD, so that part of the grid is dispatched as wavefronts retire (the
      // hardware then balances unevenly loaded SIMDs)
      const bool fast = (p.flags & HWY_C_EGO_ONLY_COLLISIONS) != 0;
      return B::pick_wpe(rollout ? l.rollout_waves_per_eu : l.waves_per_eu, [&](auto W) {
        constexpr int WPE = decltype(W)::value;
        if (rollout) return fast ? B::launch(F::template rollout_wave<WPE, false>(), l.num_envs, 64, l.extra_lds, l, a)
                                 : B::launch(F::template rollout_wave<WPE, true>(), l.num_envs, 64, l.extra_lds, l, a);
        return fast ? B::launch(F::template step_wave<WPE, false>(), l.num_envs, 64, l.extra_lds, l, a)
                    : B::launch(F::template step_wave<WPE, true>(), l.num_envs, 64, l.extra_lds, l, a);
      });
    }
    if (nw < 1 || nw > 4) return hipErrorInvalidValue;
    return B::pick_wpe(l.waves_per_eu, [&](auto W) {  // WPE = the register-allocation variant (hwy_engine.hip: waves_per_eu)
      return dispatch_1_4(nw, [&](auto V) {
        constexpr int WPE = decltype(W)::value, NW = decltype(V)::value;
        return rollout ? B::launch(F::template rollout_block<NW, WPE>(), l.num_envs, NW * 64, 0, l, a)
                       : B::launch(F::template step_block<NW, WPE>(), l.num_envs, NW * 64, 0, l, a);
      });
    });
  }
  static hipError_t reset(const P &a, const Launch &l) {
    const int nw = waves_for(F::step_params(a).N);
    if (nw < 1 || nw > 4) return hipErrorInvalidValue;
    return dispatch_1_4(nw, [&](auto V) {
      constexpr int NW = decltype(V)::value;
      return B::launch(F::template reset_block<NW>(), l.num_envs, NW * 64, 0, l, a);
    });
  }
  // the re-spawn of the environments that ended in the step launch before it (hwy_step_same_step_device).  Chosen by the STEP's
  // rule, not the reset's: the first observation of an episode must come from the code that writes it under the next-step
  // auto-reset -- the one-wavefront kernel's observe_wave where the step runs on that kernel (the register-allocation builds and
  // the shapes share it), the workgroup kernel's observe_env (the kernel beside the reset kernel, NW by the reset's rule) otherwise
  static hipError_t respawn(const P &a, const Launch &l) {
    if (wave_applies(F::step_params(a), l)) return B::launch(F::respawn_wave(), l.num_envs, 64, 0, l, a);
    const int nw = waves_for(F::step_params(a).N);
    if (nw < 1 || nw > 4) return hipErrorInvalidValue;
    return dispatch_1_4(nw, [&](auto V) {
      constexpr int NW = decltype(V)::value;
      return B::launch(F::template respawn_block<NW>(), l.num_envs, NW * 64, 0, l, a);
    });
  }
  // workgroups of the step kernel this launch would run that the device holds at once (0 = unknown)
  static int resident_blocks(const P &a, const Launch &l) {
    const StepParams &p = F::step_params(a);
    const int nw = waves_for(p.N);
    if (!wave_applies(p, l) && (nw < 1 || nw > 4)) return 0;
    return B::pick_wpe(l.waves_per_eu, [&](auto W) {
      constexpr int WPE = decltype(W)::value;
      if (wave_applies(p, l))
        return (p.flags & HWY_C_EGO_ONLY_COLLISIONS) ? B::resident(F::template step_wave<WPE, false>(), 64, l.extra_lds)
                                                     : B::resident(F::template step_wave<WPE, true>(), 64, l.extra_lds);
      // workgroup kernel: turns by workgroup (hwy_device.h: wave_turn_init_workgroup)
      return dispatch_1_4(nw, [&](auto V) { return B::resident(F::template step_block<decltype(V)::value, WPE>(), decltype(V)::value * 64, 0); });
    });
  }
};

// The selection of every family is the overload set select_step / select_reset / select_respawn / select_observe /
// select_resident_blocks<B>, chosen
// by the type of the kernel argument (StepParams, NetParams and IxParams: hwy_launch_rules.h).  Linear traffic and direct ego control:
// the one-wavefront kernel for N <= 64 (unless force_block_kernel), the workgroup kernel otherwise -- hwy_wave2.h is IDM-only.
template <typename B> hipError_t select_step(const LinearParams &a, const Launch &l, bool rollout) { return FamilyLaunch<LinearFamily, B>::step(a, l, rollout); }
template <typename B> hipError_t select_reset(const LinearParams &a, const Launch &l) { return FamilyLaunch<LinearFamily, B>::reset(a, l); }
template <typename B> hipError_t select_respawn(const LinearParams &a, const Launch &l) { return FamilyLaunch<LinearFamily, B>::respawn(a, l); }
template <typename B> int select_resident_blocks(const LinearParams &a, const Launch &l) { return FamilyLaunch<LinearFamily, B>::resident_blocks(a, l); }
template <typename B> hipError_t select_step(const DirectParams &a, const Launch &l, bool rollout) { return FamilyLaunch<DirectFamily, B>::step(a, l, rollout); }
template <typename B> hipError_t select_reset(const DirectParams &a, const Launch &l) { return FamilyLaunch<DirectFamily, B>::reset(a, l); }
template <typename B> hipError_t select_respawn(const DirectParams &a, const Launch &l) { return FamilyLaunch<DirectFamily, B>::respawn(a, l); }
template <typename B> int select_resident_blocks(const DirectParams &a, const Launch &l) { return FamilyLaunch<DirectFamily, B>::resident_blocks(a, l); }
// (the observation of a straight road does not depend on the traffic model or the ego control)
template <typename B> hipError_t select_observe(const StepParams &p, const Launch &l) {
  const int nw = waves_for(p.N);
  if (nw < 1 || nw > 4) return hipErrorInvalidValue;
  return dispatch_1_4(nw, [&](auto V) {
    constexpr int NW = decltype(V)::value;
    return B::launch(hwy_observe_kernel<NW>, l.num_envs, NW * 64, 0, l, p);
  });
}
template <typename B> hipError_t select_observe(const LinearParams &a, const Launch &l) { return select_observe<B>(a.s, l); }
template <typename B> hipError_t select_observe(const DirectParams &a, const Launch &l) { return select_observe<B>(a.s, l); }

}  // namespace hwy

// hwy_step_shapes(on): 1 = launches whose StepParams match a shape take its kernel, 0 = every launch takes the generic kernel,
// anything else = no change; returns what was in force.  hwy_last_step_shape(): the shape id of the last step launch of a
// straight-road family (0 = generic; hwy_wave.h: FastShape3 = 1, FastShape4 = 2, V0Shape4 = 3).  Process-wide, for A/B runs and tests.
extern "C" {
__attribute__((used, visibility("default"))) inline int hwy_step_shapes(int on) {
  hwy::StepShapeState &s = hwy::step_shape_state();
  const int was = s.enabled ? 1 : 0;
  if (on == 0 || on == 1) s.enabled = on == 1;
  return was;
}
__attribute__((used, visibility("default"))) inline int hwy_last_step_shape(void) { return hwy::step_shape_state().last; }
}
