// hwy_same_step.h -- gymnasium's SameStep autoreset on the device (hwy_step_same_step_device): the stash kernel that keeps the
// terminal rows of the environments that ended, and the sequence of launches one call enqueues.
//
// No step / reset / observe kernel is touched.  The step launch is the family's ordinary one with auto-reset enabled -- it writes
// done[e] = terminated | truncated -- and everything SameStep adds runs behind it on the engine's stream:
//   1  the step launch (a Lidar engine: + the trace of the state it left, so that the stash sees the terminal trace)
//   2  the mask kernel (hwy_mask.h) on that state into final_action_mask                          (if asked for)
//   3  the stash, hwy_final_kernel below: final_mask[e] = done[e]; for the environments that ended, their rows of obs, info_speed
//      and info_crashed are copied to the final planes; the rows of the others are not written at all
//   4  the family's re-spawn kernel (hwy_device.h: Begin::SameStep has the contract; hwy_wave.h, hwy_wave2.h and hwy_net.h hold the
//      forms of their step kernels, hwy_launch_family.h / hwy_launch_rules.h: select_respawn picks one by the step's rule), which
//      starts the next episode of the environments that ended, observes it into obs and clears done[e]; reward / terminated /
//      truncated stay the ending step's
//   5  a Lidar engine: the trace again (rows of environments that did not end come out as they were: the same state, the same code)
//   6  the mask kernel on the state the call leaves into action_mask                              (if asked for)
// The order is same_step_sequence's, written ONCE for hwy_engine.hip and for the CPU emulation (tests/emu/emu_same_step.cpp).
//
// The stash: one workgroup per environment.  done[e] is uniform over the workgroup -- one scalar load, and in the steady state
// about duration / (duration + 1) of the workgroups leave right behind it.  A workgroup that stays copies the environment's
// observation row ([A]..., contiguous) with one 16-byte access per thread and trip where the row allows it (a whole number of
// float4 on both sides), dword accesses otherwise: consecutive threads, consecutive addresses.
//
// Like hwy_mask.h this header includes no HIP runtime: hwy_kernels_final.hip includes <hip/hip_runtime.h> first, the CPU emulation
// its shim, hip_emu.h.  The launch rule is hwy_launch_units.h's (select_final), for both.
#pragma once

#include <stdint.h>
#include <string.h>

#include "../../include/hwy_engine.h"

namespace hwy {

#define HWY_FINAL_BLOCK 64         // threads of a workgroup for rows of at most HWY_FINAL_SMALL_FLOATS floats (Kinematics, Lidar) ...
#define HWY_FINAL_BLOCK_LARGE 256  // ... and beyond (OccupancyGrid)
#define HWY_FINAL_SMALL_FLOATS 1024

struct FinalParams {
  const uint8_t *done;          // [E] what the step launch wrote
  uint8_t *final_mask;          // [E]
  const float *obs;             // [E][row_floats]
  float *final_obs;             // [E][row_floats]
  const double *info_speed;     // [E][A], or null with its final plane
  double *final_info_speed;
  const uint8_t *info_crashed;  // [E][A], or null with its final plane
  uint8_t *final_info_crashed;
  int32_t E, A;
  int32_t row_floats;           // floats of one environment's observation: A x the per-agent length
  int32_t vec4;                 // 1: a row is a whole number of float4 and both planes are 16-byte aligned
};

// host side: what hwy_step_same_step_device refuses before any launch.  Shared by hwy_engine.hip and the CPU emulation.
inline int same_step_validate(const hwy_config &c, bool autoreset, bool has_final_obs, bool has_final_mask, const char **why) {
  *why = "";
  if (c.scenario == HWY_SCENARIO_INTERSECTION) {
    *why = "the intersection scenario keeps its next episodes pre-warmed in shadow planes keyed to the episode counter: "
           "a same-step re-spawn beside them is not supported";
    return HWY_ERR_UNSUPPORTED;
  }
  if (!autoreset) {
    *why = "auto-reset must be enabled (hwy_set_autoreset supplies base_seed and the spawn arguments)";
    return HWY_ERR_INVALID_ARG;
  }
  if (!has_final_obs || !has_final_mask) {
    *why = "final_obs and final_mask must be non-NULL";
    return HWY_ERR_INVALID_ARG;
  }
  return HWY_OK;
}

// host side: the stash's arguments of a config; obs_floats_per_agent: hwy_params.h's obs_len
inline FinalParams final_params(const hwy_config &c, size_t obs_floats_per_agent, const uint8_t *done, uint8_t *final_mask, const float *obs,
                                float *final_obs, const double *info_speed, double *final_info_speed, const uint8_t *info_crashed,
                                uint8_t *final_info_crashed) {
  FinalParams p;
  memset(&p, 0, sizeof p);
  p.done = done; p.final_mask = final_mask; p.obs = obs; p.final_obs = final_obs;
  p.info_speed = final_info_speed ? info_speed : nullptr; p.final_info_speed = info_speed ? final_info_speed : nullptr;
  p.info_crashed = final_info_crashed ? info_crashed : nullptr; p.final_info_crashed = info_crashed ? final_info_crashed : nullptr;
  p.E = c.num_envs; p.A = c.num_agents;
  p.row_floats = (int32_t)(obs_floats_per_agent * (size_t)c.num_agents);
  p.vec4 = (p.row_floats % 4 == 0 && ((uintptr_t)obs % 16 == 0) && ((uintptr_t)final_obs % 16 == 0)) ? 1 : 0;
  return p;
}

struct alignas(16) FinalVec4 { float v[4]; };  // one 16-byte access (global_load / store_dwordx4)

// BLOCK: threads per workgroup (a template so that the header can be included by several translation units)
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) hwy_final_kernel(const FinalParams p) {
  const int e = (int)blockIdx.x, i = (int)threadIdx.x;
  const uint8_t d = p.done[e];  // block-uniform
  if (i == 0) p.final_mask[e] = d;
  if (!d) return;
  const size_t row = (size_t)e * (size_t)p.row_floats;
  if (p.vec4) {
    const FinalVec4 *src = (const FinalVec4 *)(p.obs + row);
    FinalVec4 *dst = (FinalVec4 *)(p.final_obs + row);
    for (int k = i; k < p.row_floats / 4; k += BLOCK) dst[k] = src[k];
  } else {
    for (int k = i; k < p.row_floats; k += BLOCK) p.final_obs[row + k] = p.obs[row + k];
  }
  for (int a = i; a < p.A; a += BLOCK) {
    const size_t r = (size_t)e * p.A + a;
    if (p.final_info_speed) p.final_info_speed[r] = p.info_speed[r];
    if (p.final_info_crashed) p.final_info_crashed[r] = p.info_crashed[r];
  }
}

// host side: the launches of one call, in order (the list at the top).  `ops` supplies them -- step(), mask(final), stash(),
// respawn(), each returning 0 or the status the call returns; respawn() includes a Lidar engine's second trace.
template <typename Ops>
inline int same_step_sequence(Ops &&ops, bool final_action_mask, bool action_mask) {
  if (int rc = ops.step()) return rc;
  if (final_action_mask)
    if (int rc = ops.mask(true)) return rc;
  if (int rc = ops.stash()) return rc;
  if (int rc = ops.respawn()) return rc;
  if (action_mask)
    if (int rc = ops.mask(false)) return rc;
  return 0;
}

}  // namespace hwy
