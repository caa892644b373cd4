// hwy_launch_rules.h -- the rest of the selection layer of hwy_launch_family.h (same backend B, same overload set): IDM with
// meta-actions and its wide kernel (hwy_wave2.h), the road-network scenarios (hwy_net.h) and the intersection scenario (hwy_ix.h).
// Used by hwy_kernels.hip with HipBackend and by tests/emu/emu_engine.cpp with EmuBackend.  A kernel with ONE register-allocation
// build is named with that build's constant on both sides (the template parameter is a launch bound, not code).
#pragma once
#include "hwy_launch_family.h"
#include "hwy_wave2.h"
#include "hwy_net.h"
#include "hwy_ix.h"

namespace hwy {

// 64 < N <= 256 with the Kinematics observation: ONE wavefront per environment, ceil(N / 64) vehicles per thread (hwy_wave2.h).
// Two per thread (BASELINE config 3's N = 101): 245 VGPRs, 15.7 KB of LDS, two resident wavefronts per SIMD.  Three / four per thread
// (N <= 192 / 256; round 5): 338 / 436 VGPRs without a spill, 23 / 30 KB of LDS, ONE wavefront per SIMD -- the same source, bit-identical
// to the workgroup kernel (tests/test_wide_kernel.py); the workgroup kernel (hwy_device.h) remains for the OccupancyGrid observation
// with N > 64 and behind hwy_config.tune_block_kernel.
static inline bool wide_kernel_applies(const StepParams &p, const Launch &l) {
  return p.N > 64 && p.N <= 256 && p.obs_type == HWY_OBS_KINEMATICS && !l.force_block_kernel;
}
// Straight road, IDM traffic and meta-actions: the one-wavefront kernel for N <= 64, the wide kernel where it applies (one
// register-allocation variant per K: waves_per_eu does not count), the workgroup kernel otherwise or when forced
template <typename B> hipError_t select_step(const StepParams &p, const Launch &l, bool rollout) {
  if (!wide_kernel_applies(p, l)) {
    // a launch whose every structural field is that of a registered shape runs the kernel compiled for it (hwy_wave.h: FixedShape)
    if (const int shape = step_shape_of(p, l, rollout)) return launch_step_shape<B>(shape, p, l);
    return FamilyLaunch<IdmFamily, B>::step(p, l, rollout);
  }
  step_shape_state().last = 0;
  switch (waves_for(p.N)) {
    case 2: return rollout ? B::launch(hwy_rollout_wide_kernel<2, 2>, l.num_envs, 64, 0, l, p)
                           : B::launch(hwy_step_wide_kernel<2, 2>, l.num_envs, 64, 0, l, p);
    case 3: return rollout ? B::launch(hwy_rollout_wide_kernel<3, 1>, l.num_envs, 64, 0, l, p)
                           : B::launch(hwy_step_wide_kernel<3, 1>, l.num_envs, 64, 0, l, p);
    default: return rollout ? B::launch(hwy_rollout_wide_kernel<4, 1>, l.num_envs, 64, 0, l, p)
                            : B::launch(hwy_step_wide_kernel<4, 1>, l.num_envs, 64, 0, l, p);
  }
}
template <typename B> hipError_t select_reset(const StepParams &p, const Launch &l) { return FamilyLaunch<IdmFamily, B>::reset(p, l); }
// the re-spawn follows the step's rule (hwy_launch_family.h: FamilyLaunch::respawn says why): the wide kernel's where the step runs on it
template <typename B> hipError_t select_respawn(const StepParams &p, const Launch &l) {
  if (!wide_kernel_applies(p, l)) return FamilyLaunch<IdmFamily, B>::respawn(p, l);
  switch (waves_for(p.N)) {
    case 2: return B::launch(hwy_respawn_wide_kernel<2, 2>, l.num_envs, 64, 0, l, p);
    case 3: return B::launch(hwy_respawn_wide_kernel<3, 1>, l.num_envs, 64, 0, l, p);
    default: return B::launch(hwy_respawn_wide_kernel<4, 1>, l.num_envs, 64, 0, l, p);
  }
}
template <typename B> int select_resident_blocks(const StepParams &p, const Launch &l) {
  if (wide_kernel_applies(p, l)) return 0;  // (the wide kernel takes no issue-priority turns)
  return FamilyLaunch<IdmFamily, B>::resident_blocks(p, l);
}

// Road-network scenarios: one wavefront per environment; <3, true> / <1, true>: the OccupancyGrid build (its own instantiation:
// hwy_net.h, net_observe<GRID>)
template <typename B> hipError_t select_step(const NetParams &np, const Launch &l, bool rollout) {
  if (np.s.obs_type != HWY_OBS_KINEMATICS)
    return rollout ? B::launch(hwy_net_rollout_kernel<3, true>, l.num_envs, 64, 0, l, np)
                   : B::launch(hwy_net_step_kernel<3, true>, l.num_envs, 64, 0, l, np);
  return B::pick_wpe(l.waves_per_eu, [&](auto W) {
    constexpr int WPE = decltype(W)::value;
    return rollout ? B::launch(hwy_net_rollout_kernel<WPE>, l.num_envs, 64, 0, l, np)
                   : B::launch(hwy_net_step_kernel<WPE>, l.num_envs, 64, 0, l, np);
  });
}
template <typename B> hipError_t select_reset(const NetParams &np, const Launch &l) {
  if (np.s.obs_type != HWY_OBS_KINEMATICS) return B::launch(hwy_net_reset_kernel<1, true>, l.num_envs, 64, 0, l, np);
  return B::launch(hwy_net_reset_kernel<1>, l.num_envs, 64, 0, l, np);
}
template <typename B> hipError_t select_respawn(const NetParams &np, const Launch &l) {
  if (np.s.obs_type != HWY_OBS_KINEMATICS) return B::launch(hwy_net_respawn_kernel<1, true>, l.num_envs, 64, 0, l, np);
  return B::launch(hwy_net_respawn_kernel<1>, l.num_envs, 64, 0, l, np);
}
template <typename B> hipError_t select_observe(const NetParams &np, const Launch &l) {
  if (np.s.obs_type != HWY_OBS_KINEMATICS) return B::launch(hwy_net_observe_kernel<1, true>, l.num_envs, 64, 0, l, np);
  return B::launch(hwy_net_observe_kernel<1>, l.num_envs, 64, 0, l, np);
}
template <typename B> int select_resident_blocks(const NetParams &, const Launch &l) {
  return B::pick_wpe(l.waves_per_eu, [&](auto W) { return B::resident(hwy_net_step_kernel<decltype(W)::value>, 64, 0); });
}

// Intersection scenario: 32 threads for N <= 32 (64 with helper lanes), WPE 2 or 3 (158 VGPRs: 3 waves/SIMD is the most that fits);
// N > 32: 24 KB of LDS, 2 waves/SIMD.  A rollout launch (ip.s.k_steps policy steps, hwy_rollout_device) holds STEP blocks only; a
// step launch with next-episode pre-warming holds a second block per environment (hwy_ix.h: ix_prewarm)
template <typename B> hipError_t select_step(const IxParams &ip, const Launch &l, bool rollout) {
  const int grid = (!rollout && ip.shadow_meta && ip.s.autoreset && ip.s.full_step) ? 2 * l.num_envs : l.num_envs;
  if (ip.s.N > 32) return rollout ? B::launch(hwy_ix_rollout_kernel<2, 64>, grid, 64, 0, l, ip) : B::launch(hwy_ix_step_kernel<2, 64>, grid, 64, 0, l, ip);
  return B::pick_wpe(l.waves_per_eu >= 3 && l.waves_per_eu <= 4 ? 3 : 2, [&](auto W) {
    constexpr int WPE = decltype(W)::value >= 3 ? 3 : 2;
    if (ip.helpers) return rollout ? B::launch(hwy_ix_rollout_kernel<WPE, 32, 64>, grid, 64, 0, l, ip)
                                   : B::launch(hwy_ix_step_kernel<WPE, 32, 64>, grid, 64, 0, l, ip);
    return rollout ? B::launch(hwy_ix_rollout_kernel<WPE, 32>, grid, 32, 0, l, ip) : B::launch(hwy_ix_step_kernel<WPE, 32>, grid, 32, 0, l, ip);
  });
}
template <typename B> hipError_t select_reset(const IxParams &ip, const Launch &l) {
  if (ip.s.N <= 32 && ip.helpers) return B::launch(hwy_ix_reset_kernel<2, 32, 64>, l.num_envs, 64, 0, l, ip);
  if (ip.s.N <= 32) return B::launch(hwy_ix_reset_kernel<2, 32>, l.num_envs, 32, 0, l, ip);
  return B::launch(hwy_ix_reset_kernel<2, 64>, l.num_envs, 64, 0, l, ip);
}
template <typename B> hipError_t select_observe(const IxParams &ip, const Launch &l) {
  if (ip.s.N <= 32) return B::launch(hwy_ix_observe_kernel<1, 32>, l.num_envs, 32, 0, l, ip);
  return B::launch(hwy_ix_observe_kernel<1, 64>, l.num_envs, 64, 0, l, ip);
}
template <typename B> int select_resident_blocks(const IxParams &, const Launch &) { return 0; }

}  // namespace hwy
